"""fp64 restatement of the coupled multigrid cycle ``pc_type pph_cmg`` (test infrastructure only).

The hierarchy is ``oracle.dpp_mg_oracle.build_hierarchy``'s, once per field (same halving rule, rediscretised level
operators, injected masks, transfers); on top of it, per level l with n_l nodes and field-major vectors of 2 n_l entries:

* operator ``A_l = [[A11_l, C_l], [C_l^T, A22_l]]``, ``C_l = -(beta/mu) F0 M_l F1`` (M_l the level's mass matrix, F_f zeroes
  the constrained dofs of field f: rows constrained in field 0 and columns constrained in field 1 are zero);
* block diagonal ``D_l``: per node ``[[d11, d12], [d12, d22]]`` from the diagonals of A11_l, A22_l and C_l (d12 = 0 where either
  field is constrained).  Determinant from ``s1 = d11 + d12``, ``s2 = d22 + d12`` as ``s1 s2 - d12 (s1 + s2)`` - all terms
  non-negative, where ``d11 d22 - d12^2`` cancels once beta M_ii dominates;
* ``lam_l`` = largest absolute row sum of ``D_l^-1 A_l``;
* smoother: the recurrence of ``dpp_mg_oracle.chebyshev`` on [0.25 lam_l, lam_l] with ``D_l^-1`` in place of 1 / diag;
* transfers: blockdiag(P, P) and its transpose, every field with its own masks, as ``dpp_mg_oracle.vcycle`` does per field;
* coarsest level: CG on A_L under D_L^-1 to rtol 1e-12 (``dpp_oracle.pcg``'s preconditioned-norm rule, at most 500);
* a mesh that cannot be coarsened: max(steps, 2) Chebyshev steps from a zero guess;
* input entries on constrained dofs are taken as 0.

``levels_as(levels, np.longdouble)`` is the same hierarchy with dense extended-precision operators (small meshes): the drift
between the two is the restatement's own rounding error.  Hooks (``drop_coupling``, ``scalar_lam``, ``ignore_mask``) are the
mistakes the rejection tests plant.  ``cmg_grid`` / ``cmg_lanes`` restate the launch rule of perphil_amd/csrc/pph_cmg.hip.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass, replace
from typing import List, Optional, Tuple

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mg_cycle_reference as R  # noqa: E402
from oracle import dpp_mg_oracle as G  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

QUAD, TRI, HEX, TET = R.QUAD, R.TRI, R.HEX, R.TET
K1, K2, BETA, MU = R.K1, R.K2, R.BETA, R.MU
CYCLE_BOUND, FUSED_BOUND = R.CYCLE_BOUND, R.FUSED_BOUND
COARSE_MAX_IT = 500

# ---------------------------------------------------------------------------------------------------------------------
# launch rule of pph_cmg.hip, restated
# ---------------------------------------------------------------------------------------------------------------------
CMG_GRID_BLOCKS, CMG_NODE_BLOCKS, CMG_BLOCK = 2048, 1024, 256
COARSE_THREADS = 1024             # threads of k_cmg_coarse_cg on levels above 256 nodes: more nodes and its loops take several trips
CMG_COARSE_ONCHIP = 4096          # coarsest levels of at most this many nodes: CG inside one workgroup; above: host-driven


def cmg_lanes(kind: int) -> int:
    """Lanes per row of the row-walk kernels (k_cmg_row, k_cmg_setup)."""
    return 8 if R.dim_of(kind) == 3 else 4


def cmg_grid(n: int, lanes: int) -> int:
    return max(1, min(CMG_GRID_BLOCKS, -(-n * lanes // CMG_BLOCK)))


def rows_per_pass(kind: int) -> int:
    """Rows the full grid of a row-walk kernel covers in one trip of its loop."""
    return CMG_GRID_BLOCKS * CMG_BLOCK // cmg_lanes(kind)


def row_kernel_loops(kind: int, n: int) -> bool:
    return n > cmg_grid(n, cmg_lanes(kind)) * CMG_BLOCK // cmg_lanes(kind)


def node_kernel_loops(n: int) -> bool:
    """k_cmg_init / k_cmg_mask_copy: one thread per node."""
    return n > max(1, min(CMG_NODE_BLOCKS, -(-n // CMG_BLOCK))) * CMG_BLOCK


# ---------------------------------------------------------------------------------------------------------------------
# the coupled hierarchy
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class CLevel:
    n: int
    A: object            # 2n x 2n (scipy CSR, or a dense array of another precision)
    i11: np.ndarray      # D^-1 per node: [[i11, i12], [i12, i22]]
    i12: np.ndarray
    i22: np.ndarray
    lam: float
    mask: Tuple[np.ndarray, np.ndarray]     # per field, True on constrained dofs
    P: Optional[object] = None              # scalar prolongation to this level from the next coarser one
    lam_scalar: float = 0.0                 # the scalar cycle's bounds of the two blocks (their maximum)


def block_inverse(d11, d22, d12):
    """(i11, i12, i22) of [[d11, d12], [d12, d22]]^-1, determinant without cancellation."""
    s1, s2 = d11 + d12, d22 + d12
    det = s1 * s2 - d12 * (s1 + s2)
    return d22 / det, -d12 / det, d11 / det


def _finish_level(n, A11, A22, C, mask, P, lam_scalar, drop_coupling=False, scalar_lam=False) -> CLevel:
    """CLevel from the three blocks (sparse float64 or dense of any precision)."""
    dense = isinstance(A11, np.ndarray)
    if dense:
        A = np.block([[A11, C], [C.T, A22]])
        d11, d22, d12 = np.diagonal(A11).copy(), np.diagonal(A22).copy(), np.diagonal(C).copy()
    else:
        A = sp.bmat([[A11, C], [C.T, A22]], format="csr")
        d11, d22, d12 = A11.diagonal(), A22.diagonal(), C.diagonal()
    if drop_coupling:
        d12 = 0 * d12
    i11, i12, i22 = block_inverse(d11, d22, d12)
    if scalar_lam:
        lam = lam_scalar
    else:
        # rows of D^-1 A, formed block row by block row (no 2n x 2n product)
        if dense:
            top = i11[:, None] * A[:n] + i12[:, None] * A[n:]
            bot = i12[:, None] * A[:n] + i22[:, None] * A[n:]
            lam = max(np.abs(top).sum(axis=1).max(), np.abs(bot).sum(axis=1).max())
        else:
            top = sp.diags(i11) @ A[:n] + sp.diags(i12) @ A[n:]
            bot = sp.diags(i12) @ A[:n] + sp.diags(i22) @ A[n:]
            lam = float(max(abs(top).sum(axis=1).max(), abs(bot).sum(axis=1).max()))
    return CLevel(n, A, i11, i12, i22, lam, mask, P, lam_scalar)


def coupling_block(M: sp.csr_matrix, m0: np.ndarray, m1: np.ndarray, beta: float, mu: float) -> sp.csr_matrix:
    """C = -(beta/mu) F0 M F1."""
    return (sp.diags((~m0).astype(float)) @ M @ sp.diags((~m1).astype(float)) * (-(beta / mu))).tocsr()


def coupled_hierarchy(kind: int, nx: int, ny: int, nz: int, masks, k1=K1, k2=K2, beta=BETA, mu=MU, *,
                      drop_coupling: int = -1, scalar_lam: int = -1) -> List[CLevel]:
    """The coupled levels for the Dirichlet masks ``masks`` = (field 0, field 1) on the fine nodes.  The diagonal blocks, masks
    and transfers are those of ``dpp_mg_oracle.build_hierarchy`` per field (K and M of a level are assembled once here and
    shared by the three blocks; ``test_cmg_host.py`` compares with ``build_hierarchy`` itself).  ``drop_coupling`` /
    ``scalar_lam``: the level that forms D without d12 / takes lam from the scalar rule (rejection tests)."""
    dim = R.dim_of(kind)
    cells = R.level_cells(kind, nx, ny, nz)
    dims = R.level_dims(kind, nx, ny, nz)
    m = [np.asarray(masks[0], bool).copy(), np.asarray(masks[1], bool).copy()]
    out = []
    for l, (cx, cy, cz) in enumerate(cells):
        K, M = o.assemble_scalar(o.build_mesh(dim, kind, cx, cy, cz))
        blocks, lams = [], []
        for f, coefK in enumerate((k1 / mu, k2 / mu)):
            A = G.eliminate((coefK * K + (beta / mu) * M).tocsr(), m[f])
            blocks.append(A)
            lams.append(float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() / A.diagonal())))
        C = coupling_block(M.tocsr(), m[0], m[1], beta, mu)
        P = G.prolongation(kind, dims[l + 1], dims[l]) if l + 1 < len(cells) else None
        out.append(_finish_level(m[0].size, blocks[0], blocks[1], C, (m[0].copy(), m[1].copy()), P, max(lams),
                                 drop_coupling=(l == drop_coupling), scalar_lam=(l == scalar_lam)))
        if l + 1 < len(cells):
            px, py, pz = dims[l]
            for f in (0, 1):
                m3 = m[f].reshape(pz, py, px)
                m[f] = (m3[::2, ::2, ::2] if dim == 3 else m3[:, ::2, ::2]).ravel().copy()   # coarse node C <- fine node 2C
    return out


def levels_as(levels: List[CLevel], dtype) -> List[CLevel]:
    """The same hierarchy with dense operators of precision ``dtype``; blocks, inverses and bounds recomputed in it."""
    out = []
    for L in levels:
        n = L.n
        A = np.asarray(L.A.todense() if sp.issparse(L.A) else L.A).astype(dtype)
        P = None if L.P is None else np.asarray(L.P.todense()).astype(dtype)
        out.append(_finish_level(n, A[:n, :n], A[n:, n:], A[:n, n:], L.mask, P, dtype(L.lam_scalar)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cycle
# ---------------------------------------------------------------------------------------------------------------------
def dinv_apply(L: CLevel, r):
    n = L.n
    return np.concatenate([L.i11 * r[:n] + L.i12 * r[n:], L.i12 * r[:n] + L.i22 * r[n:]])


def chebyshev(L: CLevel, b, x, steps: int):
    """``dpp_mg_oracle.chebyshev`` with D^-1 in place of 1 / diag; x=None: zero first guess."""
    lo, hi = G.CHEB_LOWER * L.lam, L.lam
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    if x is None:
        x = np.zeros_like(b)
        r = b.copy()
    else:
        r = b - L.A @ x
    d = dinv_apply(L, r) / theta
    x = x + d
    for _ in range(1, steps):
        r = r - L.A @ d
        rho_new = 1.0 / (2.0 * sigma - rho)
        d = (rho_new * rho) * d + (2.0 * rho_new / delta) * dinv_apply(L, r)
        rho = rho_new
        x = x + d
    return x


def pcg(A, b, prec, rtol: float, max_it: int, atol: float = 0.0):
    """``dpp_oracle.pcg`` with its default (preconditioned) norm, in the precision of its operands: returns (x, iterations,
    converged)."""
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    res = np.sqrt(z @ z)
    tol = max(rtol * res, atol)
    if res <= tol:
        return x, 0, True
    p = z.copy()
    rz = r @ z
    for it in range(1, max_it + 1):
        Ap = A @ p
        alpha = rz / (p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        z = prec(r)
        if np.sqrt(z @ z) <= tol:
            return x, it, True
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_it, False


def coarse_solve(L: CLevel, b):
    return pcg(L.A, b, lambda v: dinv_apply(L, v), 1e-12, COARSE_MAX_IT)[0]


def _masked(v, mask):
    n = mask[0].size
    v = v.copy()
    v[:n][mask[0]] = 0
    v[n:][mask[1]] = 0
    return v


def _per_field(P, v, nin: int, transpose: bool):
    Q = P.T if transpose else P
    return np.concatenate([Q @ v[:nin], Q @ v[nin:]])


def cycle(levels: List[CLevel], b, steps: int = 2, l: int = 0, *, ignore_mask: Tuple[int, int] = (-1, -1)):
    """One coupled V-cycle.  ``ignore_mask`` = (level, field): the transfers treat that field as unconstrained on that level."""
    L = levels[l]
    if l == len(levels) - 1:
        return coarse_solve(L, b)

    def mask_of(q):
        m = levels[q].mask
        if q == ignore_mask[0]:
            m = tuple(np.zeros_like(m[f]) if f == ignore_mask[1] else m[f] for f in (0, 1))
        return m

    x = chebyshev(L, b, None, steps)
    r = _masked(b - L.A @ x, mask_of(l))
    bc = _masked(_per_field(L.P, r, L.n, True), mask_of(l + 1))
    xc = cycle(levels, bc, steps, l + 1, ignore_mask=ignore_mask)
    x = x + _masked(_per_field(L.P, xc, levels[l + 1].n, False), mask_of(l))
    return chebyshev(L, b, x, steps)


def apply_reference(levels: List[CLevel], r, steps: int = 2, **kw):
    """z = B r: entries of r on constrained dofs taken as 0, then the cycle - or max(steps, 2) Chebyshev steps from a zero
    guess where the mesh cannot be coarsened."""
    r = _masked(np.asarray(r, dtype=levels[0].i11.dtype), levels[0].mask)
    if len(levels) == 1:
        return chebyshev(levels[0], r, None, max(steps, 2))
    return cycle(levels, r, steps, **kw)


def dense_B(levels: List[CLevel], steps: int = 2) -> np.ndarray:
    """B column by column (small meshes)."""
    N = 2 * levels[0].n
    B = np.zeros((N, N))
    e = np.zeros(N)
    for j in range(N):
        e[j] = 1.0
        B[:, j] = apply_reference(levels, e, steps)
        e[j] = 0.0
    return B


def free_dofs(levels: List[CLevel]) -> np.ndarray:
    return np.nonzero(~np.concatenate(levels[0].mask))[0]


def ba_spectrum(levels: List[CLevel], steps: int = 2):
    """(eigenvalues of B A on the free rows, B on the free rows): B symmetric positive definite there, so B A is similar to
    the symmetric L^T A L with B = L L^T."""
    f = free_dofs(levels)
    B = dense_B(levels, steps)[np.ix_(f, f)]
    A = np.asarray(levels[0].A.todense())[np.ix_(f, f)]
    Bs = 0.5 * (B + B.T)
    Lc = np.linalg.cholesky(Bs)
    ev = np.linalg.eigvalsh(Lc.T @ A @ Lc)
    return ev, B


def cg_count(levels: List[CLevel], rhs, steps: int = 2, rtol: float = 1e-8, atol: float = 1e-12, max_it: int = 500):
    """CG on A_0 under the cycle (``CG_CMG_PARAMS``: preconditioned-norm test): (x, iterations, converged)."""
    return pcg(levels[0].A, rhs, lambda v: apply_reference(levels, v, steps), rtol, max_it, atol)


def sweep_contraction(levels: List[CLevel]) -> float:
    """rho(A11^-1 A12 A22^-1 A21) on the free dofs: the contraction of a fixed-stress sweep with exact block solves."""
    n = levels[0].n
    A = np.asarray(levels[0].A.todense())
    f0, f1 = np.nonzero(~levels[0].mask[0])[0], np.nonzero(~levels[0].mask[1])[0]
    A11, A22 = A[np.ix_(f0, f0)], A[np.ix_(n + f1, n + f1)]
    A12, A21 = A[np.ix_(f0, n + f1)], A[np.ix_(n + f1, f0)]
    T = np.linalg.solve(A11, A12 @ np.linalg.solve(A22, A21))
    return float(np.abs(np.linalg.eigvals(T)).max())


# ---------------------------------------------------------------------------------------------------------------------
# probing vectors and masks
# ---------------------------------------------------------------------------------------------------------------------
def probe_vectors(levels: List[CLevel], seed: int, random_count: int = 1):
    """``mg_cycle_reference.probe_vectors``' construction applied to both fields: random vectors and, per level l,
    r = A_0 P_0 ... P_{l-1} e with e random on level l (0 on constrained entries), scaled to max |r| = 1."""
    rng = np.random.default_rng(seed)
    out = []
    for q in range(random_count):
        out.append((f"random {q}", _masked(rng.standard_normal(2 * levels[0].n), levels[0].mask)))
    for l in range(1, len(levels)):
        e = _masked(rng.standard_normal(2 * levels[l].n), levels[l].mask)
        for q in range(l - 1, -1, -1):
            e = _masked(_per_field(levels[q].P, e, levels[q + 1].n, False), levels[q].mask)
        r = _masked(levels[0].A @ e, levels[0].mask)
        out.append((f"level {l}", r / abs(r).max()))
    return out


def boundary_masks(kind: int, nx: int, ny: int, nz: int = 0):
    """Both fields constrained on the whole boundary."""
    n = R.level_nodes(kind, nx, ny, nz)[0]
    m = R.mask_of(n, R.dirichlet_nodes(kind, nx, ny, nz, 1))
    return m, m.copy()


def mixed_nodes(kind: int, nx: int, ny: int, nz: int = 0, second: bool = False):
    """Different Dirichlet sets per field: field 0 on the whole boundary; field 1 on two sides (x = 0 and y = 0; `second`:
    x = 1 and y = 1) plus a few interior nodes - some on the coarse lattices, some not.  Returns the node arrays."""
    i, j, k = R.node_ijk(kind, nx, ny, nz)
    dim = R.dim_of(kind)
    b0 = R.dirichlet_nodes(kind, nx, ny, nz, 1)
    sides = ((i == nx) | (j == ny)) if second else ((i == 0) | (j == 0))
    inside = np.zeros_like(sides)
    picks = [(0.5, 0.5, 0.5, 4), (0.25, 0.75, 0.5, 2), (0.7, 0.3, 0.4, 1)] if not second else [(0.5, 0.25, 0.5, 4), (0.3, 0.6, 0.6, 1)]
    for fx, fy, fz, q in picks:
        a, b, c = (int(round(f * m / q)) * q for f, m in ((fx, nx), (fy, ny), (fz, nz if dim == 3 else 0)))
        if 0 < a < nx and 0 < b < ny and (dim == 2 or 0 < c < nz):
            inside |= (i == a) & (j == b) & ((k == c) if dim == 3 else True)
    if second:
        # the first field gets interior nodes too, and loses one side
        i0 = np.zeros_like(sides)
        a, b, c = nx // 2, (ny // 4) * 2, (nz // 2 if dim == 3 else 0)
        i0 |= (i == a) & (j == b) & ((k == c) if dim == 3 else True)
        full = np.zeros_like(sides)
        full[b0] = True
        return np.nonzero((full & (i != 0)) | i0)[0], np.nonzero(sides | inside)[0]
    return b0, np.nonzero(sides | inside)[0]


def masks_from_nodes(n: int, nodes) -> Tuple[np.ndarray, np.ndarray]:
    return R.mask_of(n, nodes[0]), R.mask_of(n, nodes[1])


def rel_err(z, ref) -> float:
    return float(abs(z - ref).max() / abs(ref).max())
