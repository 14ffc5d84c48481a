"""NumPy / SciPy restatement of the transient DPP model on top of ``oracle.dpp_oracle`` (``build_mesh``, ``assemble_scalar``,
``boundary_nodes``), for the tests of ``perphil_amd/csrc/pph_transient.hip``.

Model, with a storage coefficient S_f > 0 per network and Dirichlet data constant in time::

    S1 dp1/dt - div(k1/mu grad p1) + beta/mu (p1 - p2) = 0
    S2 dp2/dt - div(k2/mu grad p2) - beta/mu (p1 - p2) = 0

Theta scheme (1/2 <= theta <= 1) in delta form, F the projection that zeroes the constrained dofs::

    (Sigma M / dt + theta A) d = -F A_unel p^n,   p^{n+1} = p^n + d,   d = 0 on constrained dofs

``A_unel = [[a K + b M, -b M], [-b M, c K + b M]]`` (a, b, c = k1/mu, beta/mu, k2/mu) is the un-eliminated operator, ``A`` its
Dirichlet-eliminated form (unit rows on constrained dofs).  The step operator is a steady operator with PER-FIELD mass
coefficients: ``shifted_blocks(theta k1, theta k2, theta beta, mu, S1/dt, S2/dt)``.

Closed form (quadrilaterals and hexahedra, homogeneous Dirichlet data on the whole boundary): the nodal
``phi = prod_e sin(pi x_e)`` is an eigenvector of K and of M.  Per direction, with h = 1 / n_e, the 1-D eigenvalues are
``k1d = (2 - 2 cos(pi h)) / h`` and ``m1d = h (4 + 2 cos(pi h)) / 6``; ``lam_K = sum_d k1d_d prod_{e != d} m1d_e``,
``lam_M = prod_e m1d_e`` (equal spacings: ``dim k1d m1d^(dim-1)`` and ``m1d^dim``).  ``(c1, c2) phi`` then evolves exactly by
the 2 x 2 map ``G = (S lam_M / dt + theta Ah)^-1 (S lam_M / dt - (1 - theta) Ah)``,
``Ah = [[a lam_K + b lam_M, -b lam_M], [-b lam_M, c lam_K + b lam_M]]``.  On triangles and tetrahedra phi is NOT an
eigenvector of M: simplices are pinned by the restatement alone.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import dpp_oracle as o  # noqa: E402

EPS = float(np.finfo(np.float64).eps)


@dataclass
class Coefs:
    k1: float = 1.0
    k2: float = 0.01
    beta: float = 1.0
    mu: float = 1.0

    @property
    def abc(self) -> Tuple[float, float, float]:
        return self.k1 / self.mu, self.beta / self.mu, self.k2 / self.mu


def scalar_matrices(dim: int, kind: int, nx: int, ny: int, nz: int = 0):
    """(mesh, K, M) of the oracle."""
    om = o.build_mesh(dim, kind, nx, ny, nz)
    K, M = o.assemble_scalar(om)
    return om, K.tocsr(), M.tocsr()


def masks_of(n: int, nodes0, nodes1) -> Tuple[np.ndarray, np.ndarray]:
    m0, m1 = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    m0[np.asarray(nodes0, dtype=np.int64)] = True
    m1[np.asarray(nodes1, dtype=np.int64)] = True
    return m0, m1


def unel_operator(K, M, cf: Coefs, sigma=(0.0, 0.0)) -> sp.csr_matrix:
    """[[a K + (b + sigma1) M, -b M], [-b M, c K + (b + sigma2) M]] without Dirichlet rows."""
    a, b, c = cf.abc
    return sp.bmat([[a * K + (b + sigma[0]) * M, -b * M], [-b * M, c * K + (b + sigma[1]) * M]], format="csr")


def shifted_blocks(K, M, cf: Coefs, sigma, masks, g):
    """The Dirichlet-eliminated blocks with per-field mass coefficients and the lifted right-hand side:
    returns (A11, A22, A12, A21, rhs, u0); rhs = -F A_shifted,unel u0: 0 on constrained dofs, whose rows are unit rows (the
    convention of ``oracle.dpp_oracle.build_system``: the solve is for the correction, the solution adds u0)."""
    n = K.shape[0]
    A = unel_operator(K, M, cf, sigma)
    con = np.concatenate(masks)
    u0 = np.where(con, np.concatenate(g), 0.0)
    F = sp.diags((~con).astype(np.float64))
    Ae = (F @ A @ F + sp.diags(con.astype(np.float64))).tocsr()
    rhs = -(F @ (A @ u0))
    return Ae[:n, :n].tocsr(), Ae[n:, n:].tocsr(), Ae[:n, n:].tocsr(), Ae[n:, :n].tocsr(), rhs, u0


def step_rhs(K, M, cf: Coefs, masks, p) -> np.ndarray:
    """b = -F A_unel p."""
    r = -(unel_operator(K, M, cf) @ p)
    r[np.concatenate(masks)] = 0.0
    return r


def abs_bound(K, M, cf: Coefs, p) -> np.ndarray:
    """(|A_unel| |p|)_i, componentwise: what a sum of the row's terms can lose to rounding, per unit of eps."""
    return abs(unel_operator(K, M, cf)) @ np.abs(p)


def theta_steps(K, M, cf: Coefs, storage, theta: float, dt: float, masks, g, p0, nsteps: int, steady_tol: float = 0.0):
    """Direct theta stepping (``splu`` of the step operator).  Returns (states [steps_done + 1][2n] with the constrained
    entries of p0 overwritten by g, rhs norms, increment norms)."""
    n = K.shape[0]
    con = np.concatenate(masks)
    sig = (storage[0] / dt, storage[1] / dt)
    step_cf = Coefs(theta * cf.k1, theta * cf.k2, theta * cf.beta, cf.mu)
    A11, A22, A12, A21, _, _ = shifted_blocks(K, M, step_cf, sig, masks, (np.zeros(n), np.zeros(n)))
    lu = spla.splu(sp.bmat([[A11, A12], [A21, A22]], format="csc"))
    p = np.where(con, np.concatenate(g), np.asarray(p0, dtype=np.float64))
    states, bn, dn = [p.copy()], [], []
    for _ in range(nsteps):
        b = step_rhs(K, M, cf, masks, p)
        nb = float(np.linalg.norm(b))
        if steady_tol > 0.0 and nb <= steady_tol * (bn[0] if bn else nb):
            break
        d = lu.solve(b) if nb > 0.0 else np.zeros_like(b)
        d[con] = 0.0
        p = p + d
        bn.append(nb)
        dn.append(float(np.linalg.norm(d)))
        states.append(p.copy())
    return states, np.array(bn), np.array(dn)


# -- closed form (tensor-product cells) -------------------------------------------------------------------------------
def sine_mode(om) -> np.ndarray:
    return np.prod(np.sin(np.pi * om.coords), axis=1)


def mode_eigenvalues(dim: int, nx: int, ny: int, nz: int = 0) -> Tuple[float, float]:
    """(lam_K, lam_M) of the sine mode on Q1 cells."""
    nd = [nx, ny, nz][:dim]
    k1d = [(2.0 - 2.0 * np.cos(np.pi / q)) * q for q in nd]
    m1d = [(4.0 + 2.0 * np.cos(np.pi / q)) / (6.0 * q) for q in nd]
    lam_m = float(np.prod(m1d))
    lam_k = float(sum(k1d[d] * np.prod([m1d[e] for e in range(dim) if e != d]) for d in range(dim)))
    return lam_k, lam_m


def amplification(lam_k: float, lam_m: float, cf: Coefs, storage, theta: float, dt: float) -> np.ndarray:
    a, b, c = cf.abc
    Ah = np.array([[a * lam_k + b * lam_m, -b * lam_m], [-b * lam_m, c * lam_k + b * lam_m]])
    Sm = np.diag(np.asarray(storage, dtype=np.float64)) * lam_m / dt
    return np.linalg.solve(Sm + theta * Ah, Sm - (1.0 - theta) * Ah)


def closed_form_amplitudes(G: np.ndarray, c0, nsteps: int) -> List[np.ndarray]:
    out = [np.asarray(c0, dtype=np.float64)]
    for _ in range(nsteps):
        out.append(G @ out[-1])
    return out


# -- the matrix-free step kernel (k_step_rhs, pph_transient.hip), restated ----------------------------------------------
STEP_BLOCK, STEP_MAX_BLOCKS = 256, 2048      # launch rule: min(ceil(n / 256), 2048) workgroups of 256 nodes, grid-stride
_SUBCELLS = {o.CELL_TRI: [(0, 1, 2), (1, 3, 2)],
             o.CELL_TET: [(0, 1, 3, 7), (0, 1, 7, 5), (0, 5, 7, 4), (0, 3, 2, 7), (0, 6, 4, 7), (0, 2, 6, 7)]}


def step_kernel_loops(n: int) -> bool:
    """More nodes than one pass of the kernel's grid covers."""
    return n > min(-(-n // STEP_BLOCK), STEP_MAX_BLOCKS) * STEP_BLOCK


def box_matrices(kind: int, nd) -> Tuple[np.ndarray, np.ndarray]:
    """(KB, MB) [corner a][corner b], corners x + 2y + 4z: the stiffness and mass matrix of ONE box of the uniform mesh with
    nd cells per direction, in closed form (step_box_tables)."""
    dim = len(nd)
    nc = 1 << dim
    vol = 1.0 / float(np.prod(nd))
    KB, MB = np.zeros((nc, nc)), np.zeros((nc, nc))
    if kind in (o.CELL_QUAD, o.CELL_HEX):
        S = np.array([[1.0, -1.0], [-1.0, 1.0]])
        Mm = np.array([[2.0, 1.0], [1.0, 2.0]]) / 6.0
        for a in range(nc):
            for b in range(nc):
                ab = [((a >> e) & 1, (b >> e) & 1) for e in range(dim)]
                MB[a, b] = vol * np.prod([Mm[i, j] for i, j in ab])
                KB[a, b] = vol * sum(nd[d] ** 2 * np.prod([(S if e == d else Mm)[ab[e]] for e in range(dim)]) for d in range(dim))
        return KB, MB
    subs = _SUBCELLS[kind]
    vc = vol / len(subs)
    for v in subs:
        for d in range(dim):
            lo, up = [(q, t) for q in range(dim + 1) for t in range(dim + 1) if v[t] == (v[q] | (1 << d)) and v[t] != v[q]][0]
            e = np.zeros(dim + 1)
            e[up], e[lo] = 1.0, -1.0
            for r in range(dim + 1):
                for s in range(dim + 1):
                    KB[v[r], v[s]] += vc * nd[d] ** 2 * e[r] * e[s]
        for r in range(dim + 1):
            for s in range(dim + 1):
                MB[v[r], v[s]] += vc * (2.0 if r == s else 1.0) / ((dim + 1) * (dim + 2))
    return KB, MB


def matfree_scalar_matrices(kind: int, nx: int, ny: int, nz: int = 0):
    """(K, M) as the step kernel forms them: every node gathers the rows of the box matrices of its incident boxes; a box
    outside the mesh is skipped by index arithmetic."""
    dim = 2 if kind in (o.CELL_QUAD, o.CELL_TRI) else 3
    nd = [nx, ny, nz][:dim]
    pd = [q + 1 for q in nd] + [1] * (3 - dim)
    n = int(np.prod(pd))
    KB, MB = box_matrices(kind, nd)
    idx = np.arange(n)
    ijk = [idx % pd[0], (idx // pd[0]) % pd[1], idx // (pd[0] * pd[1])]
    stride = [1, pd[0], pd[0] * pd[1]]
    rows, cols, kv, mv = [], [], [], []
    for a in range(1 << dim):
        ok = np.ones(n, dtype=bool)
        for e in range(dim):   # the node is corner a_e of the box along e: the box below exists from 1 on, the box above up to n_e - 1
            ok &= (ijk[e] > 0) if (a >> e) & 1 else (ijk[e] < nd[e])
        for b in range(1 << dim):
            off = sum((((b >> e) & 1) - ((a >> e) & 1)) * stride[e] for e in range(dim))
            rows.append(idx[ok]); cols.append(idx[ok] + off)
            kv.append(np.full(int(ok.sum()), KB[a, b])); mv.append(np.full(int(ok.sum()), MB[a, b]))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    K = sp.csr_matrix((np.concatenate(kv), (rows, cols)), shape=(n, n))
    M = sp.csr_matrix((np.concatenate(mv), (rows, cols)), shape=(n, n))
    return K, M


# -- coupled hierarchy with per-field mass coefficients (the restatement behind pc_type pph_cmg on a shifted system) --------
def coupled_hierarchy_shifted(kind: int, nx: int, ny: int, nz: int, masks, cf: Coefs, sigma):
    """``cmg_reference.coupled_hierarchy`` with A_ff = coefK_f K + (beta/mu + sigma_f) M on every level; the coupling stays
    -(beta/mu) F0 M F1."""
    import cmg_reference as C
    import mg_cycle_reference as R
    from oracle import dpp_mg_oracle as G

    dim = R.dim_of(kind)
    cells, dims = R.level_cells(kind, nx, ny, nz), R.level_dims(kind, nx, ny, nz)
    a, b, c = cf.abc
    m = [np.asarray(masks[0], bool).copy(), np.asarray(masks[1], bool).copy()]
    out = []
    for l, (cx, cy, cz) in enumerate(cells):
        K, M = o.assemble_scalar(o.build_mesh(dim, kind, cx, cy, cz))
        blocks, lams = [], []
        for f, coefK in enumerate((a, c)):
            A = G.eliminate((coefK * K + (b + sigma[f]) * M).tocsr(), m[f])
            blocks.append(A)
            lams.append(float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() / A.diagonal())))
        Cb = C.coupling_block(M.tocsr(), m[0], m[1], cf.beta, cf.mu)
        P = G.prolongation(kind, dims[l + 1], dims[l]) if l + 1 < len(cells) else None
        out.append(C._finish_level(m[0].size, blocks[0], blocks[1], Cb, (m[0].copy(), m[1].copy()), P, max(lams)))
        if l + 1 < len(cells):
            px, py, pz = dims[l]
            for f in (0, 1):
                m3 = m[f].reshape(pz, py, px)
                m[f] = (m3[::2, ::2, ::2] if dim == 3 else m3[:, ::2, ::2]).ravel().copy()
    return out
