"""References, probing vectors and restated launch rules for the CG-1 multigrid cycle tests (test infrastructure only).

* ``cycle`` restates ``oracle.dpp_mg_oracle.vcycle`` with the hooks the rejection tests need (a level's mask dropped, the
  smoother bound of the next level, a skipped post-smoothing, a loose or a direct coarsest solve, other operators inside the
  smoother); without hooks it is ``vcycle`` bit for bit (``test_mg_cycle_host.py``).  ``apply_reference`` adds the rule of a
  mesh that cannot be coarsened (max(steps, 2) Chebyshev steps, as ``pmg_restatement.cycle`` states it).
* ``matfree_hierarchy``: the same hierarchy for uniform quadrilaterals / hexahedra without a matrix.  K and M are Kronecker
  sums of the 1D P1 stiffness and mass tridiagonals; the operator is applied axis by axis, elimination is a mask
  (A_e x = x on constrained rows, (A (x off the mask)) elsewhere), the diagonal and the bound lam = max row sum of |D^-1 A_e|
  come from the stencil coefficients (outer products of the 1D diagonals, formed one offset at a time and not kept: 27
  arrays of a 161^3 level would be 0.9 GB), the transfers are 1D interpolations applied per axis.
* ``probe_vectors``: a random vector and, for every level l, r = A_0 P_0 ... P_{l-1} e with a random e on level l, so that
  an error made on level l is not hidden under the fine level's.
* ``level_nodes``, ``tail_begin``, ``tail_lds``, ``mg_grid``: the launch rules of ``perphil_amd/csrc/pph_mg.hip``
  (``mg_setup``'s halving rule, ``mg_tail_begin``, ``mg_tail_lds``, ``mg_grid``) restated, so that a test can assert the
  branch its mesh reaches.
"""
from __future__ import annotations

import os
import sys
from dataclasses import replace
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import dpp_mg_oracle as G  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

QUAD, TRI, HEX, TET = o.CELL_QUAD, o.CELL_TRI, o.CELL_HEX, o.CELL_TET
KIND_NAME = {QUAD: "quad", TRI: "tri", HEX: "hex", TET: "tet"}
K1, K2, BETA, MU = 1.0, 0.01, 1.0, 1.0      # the coefficients of the cycle tests (k1 / k2 = 100 as the benchmark's)


def dim_of(kind: int) -> int:
    return 2 if kind in (QUAD, TRI) else 3


# ---------------------------------------------------------------------------------------------------------------------
# launch rules of pph_mg.hip, restated
# ---------------------------------------------------------------------------------------------------------------------
MG_TAIL_MAX = 4
MG_TAIL_ROWS = 1024
MG_TAIL_MATPOOL = 6144
MG_TAIL_ROWS_DEFAULT = 5000        # default of option mg_tail_rows
MG_GRID_BLOCKS, MG_BLOCK = 2048, 256
MG_GRID_THREADS = MG_GRID_BLOCKS * MG_BLOCK   # 524 288: more work items than this and a transfer kernel loops
COARSE_ONCHIP_ROWS = 4096          # coarsest level without a tail: one-workgroup CG up to here, host-driven CG above


def sell_slots(kind: int) -> int:
    return {QUAD: 9, TRI: 7, HEX: 27, TET: 15}[kind]


def level_cells(kind: int, nx: int, ny: int, nz: int = 0) -> List[Tuple[int, int, int]]:
    """Cells per direction of every level: halve while every direction is even and keeps >= 2 cells."""
    dim = dim_of(kind)
    nz = nz if dim == 3 else 0
    out = [(nx, ny, nz)]
    while nx % 2 == 0 and ny % 2 == 0 and (dim == 2 or nz % 2 == 0) and nx // 2 >= 2 and ny // 2 >= 2 and (dim == 2 or nz // 2 >= 2):
        nx, ny, nz = nx // 2, ny // 2, nz // 2
        out.append((nx, ny, nz))
    return out


def level_dims(kind: int, nx: int, ny: int, nz: int = 0) -> List[Tuple[int, int, int]]:
    """Nodes per direction (px, py, pz) of every level."""
    dim = dim_of(kind)
    return [(cx + 1, cy + 1, cz + 1 if dim == 3 else 1) for cx, cy, cz in level_cells(kind, nx, ny, nz)]


def level_nodes(kind: int, nx: int, ny: int, nz: int = 0) -> List[int]:
    return [px * py * pz for px, py, pz in level_dims(kind, nx, ny, nz)]


def tail_lds(ns: Sequence[int], S: int) -> int:
    """``mg_tail_lds``: LDS bytes of k_mg_tail for these level sizes, 0 when they do not fit its limits."""
    nl = len(ns)
    if nl < 1 or nl > MG_TAIL_MAX or ns[0] > MG_TAIL_ROWS:
        return 0
    d = sum(3 * n for n in ns) + 2 * ns[-1]
    mk = sum((n + 7) & ~7 for n in ns)
    mat = sum(S * n for n in ns[1:])
    if mat > MG_TAIL_MATPOOL:
        return 0
    return (d + mat) * 8 + mk


def tail_begin(ns: Sequence[int], kind: int, tail_rows: int = MG_TAIL_ROWS_DEFAULT, coarse_on_device: bool = True) -> int:
    """``mg_tail_begin`` on one context with stencil-ELL levels: first level of the tail, len(ns) when there is none."""
    nlev = len(ns)
    if not coarse_on_device:
        return nlev
    cap = min(tail_rows, MG_TAIL_ROWS)
    lt = nlev
    for l in range(nlev - 1, 0, -1):
        if ns[l] > cap or nlev - l > MG_TAIL_MAX or tail_lds(ns[l:], sell_slots(kind)) == 0:
            break
        lt = l
    return lt


def mg_grid(n: int) -> int:
    return max(1, min(MG_GRID_BLOCKS, -(-n // MG_BLOCK)))


def loops(n_items: int) -> bool:
    """A NODE_LOOP over n_items work items launched with mg_grid(.) blocks makes more than one trip."""
    return n_items > mg_grid(n_items) * MG_BLOCK


def q1_pairs(dims: Tuple[int, int, int]) -> int:
    """Work items of k_prolong_to_q1 on a level: pairs of fine nodes along x."""
    px, py, pz = dims
    return ((px + 1) >> 1) * py * pz


def branch_of(kind: int, nx: int, ny: int, nz: int = 0, tail_rows: int = MG_TAIL_ROWS_DEFAULT, coarse_on_device: bool = True) -> dict:
    """What one fused cycle on this mesh launches, from the restated rules."""
    ns = level_nodes(kind, nx, ny, nz)
    nlev = len(ns)
    lt = tail_begin(ns, kind, tail_rows, coarse_on_device)
    d = {"levels": ns, "nlev": nlev, "lt": lt, "NL": nlev - lt if lt < nlev else 0}
    if nlev == 1:
        d["coarsest"] = "chebyshev only"
    elif lt < nlev:
        d["coarsest"] = "tail, one-wave CG" if ns[-1] <= 64 else "tail, workgroup CG"
    elif ns[-1] <= COARSE_ONCHIP_ROWS and coarse_on_device:
        d["coarsest"] = "k_coarse_cg_sell"
    else:
        d["coarsest"] = "pph_cg_jacobi"
    return d


# ---------------------------------------------------------------------------------------------------------------------
# Dirichlet sets that are not the box surface
# ---------------------------------------------------------------------------------------------------------------------
def node_ijk(kind: int, nx: int, ny: int, nz: int = 0):
    px, py, pz = level_dims(kind, nx, ny, nz)[0]
    idx = np.arange(px * py * pz)
    return idx % px, (idx // px) % py, idx // (px * py)


def dirichlet_nodes(kind: int, nx: int, ny: int, nz: int = 0, variant: int = 0, field: int = 0) -> np.ndarray:
    """variant 0: the boundary without the side x = 1 (natural there) plus a few constrained nodes INSIDE the domain - some at
    lattice points that survive two coarsenings, some at odd ones, other ones per field; variant 1: the whole boundary."""
    dim = dim_of(kind)
    i, j, k = node_ijk(kind, nx, ny, nz)
    bnd = (i == 0) | (i == nx) | (j == 0) | (j == ny)
    if dim == 3:
        bnd |= (k == 0) | (k == nz)
    if variant == 1:
        return np.nonzero(bnd)[0]
    bnd &= i != nx
    inside = np.zeros_like(bnd)
    picks = [(0.5, 0.5, 0.5, 4), (0.25, 0.5, 0.75, 2), (0.7, 0.3, 0.4, 1)] if field == 0 else \
            [(0.5, 0.25, 0.5, 4), (0.75, 0.75, 0.25, 2), (0.3, 0.6, 0.6, 1), (0.45, 0.4, 0.3, 1)]
    for fx, fy, fz, q in picks:
        # the lattice point nearest to the fraction on the lattice of spacing q (4: also a node two levels down)
        a, b, c = (int(round(f * n / q)) * q for f, n in ((fx, nx), (fy, ny), (fz, nz if dim == 3 else 0)))
        if 0 < a < nx and 0 < b < ny and (dim == 2 or 0 < c < nz):
            inside |= (i == a) & (j == b) & ((k == c) if dim == 3 else True)
    return np.nonzero(bnd | inside)[0]


def dirichlet_values(kind: int, nx: int, ny: int, nz: int, nodes: np.ndarray, field: int) -> np.ndarray:
    i, j, k = node_ijk(kind, nx, ny, nz)
    x, y, z = i[nodes] / nx, j[nodes] / ny, (k[nodes] / nz if dim_of(kind) == 3 else 0.0 * nodes)
    return np.exp(x) * np.sin(3 * y) + z if field == 0 else np.cos(2 * x) + y * y - 0.5 * z


def mask_of(n: int, nodes: np.ndarray) -> np.ndarray:
    m = np.zeros(n, bool)
    m[nodes] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the cycle, with hooks
# ---------------------------------------------------------------------------------------------------------------------
def _coarse(lv, b, rtol, direct):
    if direct:
        return spla.spsolve(sp.csc_matrix(lv.A), b)
    return o.pcg(lv.A, b, lambda v: lv.dinv * v, rtol=rtol, atol=1e-300, max_it=500).x


def cycle(levels, b, steps: int = 1, l: int = 0, *, drop_mask: int = -1, lam_from_next: int = -1, skip_post: int = -1,
          coarse_rtol: float = 1e-12, coarse_direct: bool = False, smooth_A: Optional[list] = None) -> np.ndarray:
    """``dpp_mg_oracle.vcycle``; hooks: ``drop_mask`` = level whose mask the transfers ignore, ``lam_from_next`` = level that
    smooths with the next level's bound, ``skip_post`` = level without post-smoothing, ``coarse_rtol`` / ``coarse_direct`` =
    the coarsest solve, ``smooth_A`` = per level the operator of the smoother and residual products (None: the level's)."""
    kw = dict(drop_mask=drop_mask, lam_from_next=lam_from_next, skip_post=skip_post, coarse_rtol=coarse_rtol,
              coarse_direct=coarse_direct, smooth_A=smooth_A)
    lv = levels[l]
    if l == len(levels) - 1:
        return _coarse(lv, b, coarse_rtol, coarse_direct)
    sm = lv
    if smooth_A is not None and smooth_A[l] is not None:
        sm = replace(sm, A=smooth_A[l])
    if l == lam_from_next:
        sm = replace(sm, lam=levels[l + 1].lam)
    mf = np.zeros_like(lv.mask) if l == drop_mask else lv.mask
    mc = np.zeros_like(levels[l + 1].mask) if l + 1 == drop_mask else levels[l + 1].mask
    x = G.chebyshev(sm, b, None, steps)
    r = b - sm.A @ x
    r[mf] = 0.0
    bc = lv.P.T @ r
    bc[mc] = 0.0
    xc = cycle(levels, bc, steps, l + 1, **kw)
    corr = lv.P @ xc
    corr[mf] = 0.0
    x = x + corr
    if l == skip_post:
        return x
    return G.chebyshev(sm, b, x, steps)


def apply_reference(levels, r: np.ndarray, steps: int, **kw) -> np.ndarray:
    """One application of the block preconditioner ``mg`` to r (0 on constrained entries): the V-cycle, or max(steps, 2)
    Chebyshev steps from a zero guess where the mesh cannot be coarsened."""
    if len(levels) == 1:
        return G.chebyshev(levels[0], r, None, max(steps, 2))
    return cycle(levels, r, steps, **kw)


def fp32_operators(levels) -> list:
    """Level operators rounded to fp32 (option mg_fp32: the smoother's and residual products read fp32 values)."""
    out = []
    for lv in levels:
        A = lv.A.copy()
        A.data = A.data.astype(np.float32).astype(np.float64)
        out.append(A)
    return out


def permuted(levels, seed: int):
    """The same hierarchy under a random renumbering of every level; returns (levels', permutation of level 0)."""
    rng = np.random.default_rng(seed)
    perms = [rng.permutation(lv.mask.size) for lv in levels]
    out = []
    for l, lv in enumerate(levels):
        p = perms[l]
        A = lv.A.tocsr()[p][:, p].tocsr()
        P = None if lv.P is None else lv.P.tocsr()[p][:, perms[l + 1]].tocsr()
        out.append(G.Level(A, lv.dinv[p], lv.mask[p], lv.lam, P))
    return out, perms[0]


def apply_permuted(plevels, perm, r, steps: int, **kw) -> np.ndarray:
    z = np.empty_like(r)
    z[perm] = apply_reference(plevels, r[perm], steps, **kw)
    return z


def with_transfer_weight(levels, dims, l: int, rel: float = 1e-6):
    """Copy of the hierarchy whose transfer between levels l and l + 1 has ONE weight off by the factor (1 + rel): the tap
    towards +x of the odd fine nodes on the face x = max of level l (the natural side of ``dirichlet_nodes`` variant 0)."""
    px, py, pz = dims[l]
    pxc = dims[l + 1][0]
    P = levels[l].P.tocoo()
    fi, ci = P.row % px, P.col % pxc
    hit = (fi == px - 2) & (ci == pxc - 1) & ((P.row // px) % py % 2 == 0) & ((P.row // (px * py)) % 2 == 0)
    assert hit.any()
    data = P.data.copy()
    data[hit] *= 1.0 + rel
    out = list(levels)
    out[l] = replace(levels[l], P=sp.coo_matrix((data, (P.row, P.col)), shape=P.shape).tocsr())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# probing vectors and the comparison
# ---------------------------------------------------------------------------------------------------------------------
def probe_vectors(levels, seed: int, random_count: int = 1):
    """[(name, r)]: r is 0 on the constrained entries of level 0.  'level l': r = A_0 P_0 ... P_{l-1} e, e random on level l
    (0 on its constrained entries), scaled to max |r| = 1."""
    rng = np.random.default_rng(seed)
    m0 = levels[0].mask
    out = []
    for q in range(random_count):
        r = rng.standard_normal(m0.size)
        r[m0] = 0.0
        out.append((f"random {q}", r))
    for l in range(1, len(levels)):
        e = rng.standard_normal(levels[l].mask.size)
        e[levels[l].mask] = 0.0
        for q in range(l - 1, -1, -1):
            e = levels[q].P @ e
            e[levels[q].mask] = 0.0
        r = levels[0].A @ e
        r[m0] = 0.0
        out.append((f"level {l}", r / abs(r).max()))
    return out


CYCLE_BOUND = 1e-10      # max |z - ref| <= CYCLE_BOUND max |ref|: the bound of tests/test_pmg_gpu.py::_check_cycle
FUSED_BOUND = 1e-12      # fused against general cycle on one context, as there


def rel_err(z: np.ndarray, ref: np.ndarray) -> float:
    return float(abs(z - ref).max() / abs(ref).max())


def worst_error(apply: Callable[[np.ndarray], np.ndarray], reference: Callable[[np.ndarray], np.ndarray], vectors):
    """(worst relative error over the probing vectors, its name, per-vector list)."""
    errs = [(rel_err(apply(r), reference(r)), name) for name, r in vectors]
    w = max(errs)
    return w[0], w[1], errs


# ---------------------------------------------------------------------------------------------------------------------
# k iterations of PCG without a test (inner_norm 2)
# ---------------------------------------------------------------------------------------------------------------------
def pcg_fixed(A, b: np.ndarray, prec: Callable[[np.ndarray], np.ndarray], k: int, first_rz_factor: float = 1.0) -> np.ndarray:
    """Exactly k CG iterations from a zero guess, no convergence test (``dpp_oracle.pcg(norm="none")`` restated);
    ``first_rz_factor`` scales r.z of the first iteration (rejection tests)."""
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = z.copy()
    rz = float(np.dot(r, z)) * first_rz_factor
    for it in range(k):
        Ap = A @ p
        alpha = rz / float(np.dot(p, Ap))
        x += alpha * p
        r -= alpha * Ap
        if it == k - 1:
            break
        z = prec(r)
        rz_new = float(np.dot(r, z))
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x


def picard_sweep(A11, A22, A21, rhs: np.ndarray, prec1, prec2, k: int, first_rz_factor: float = 1.0) -> np.ndarray:
    """du of one Picard sweep whose block solves are k PCG iterations each: block 1 from rhs[:n], block 2 from
    rhs[n:] - A21 x1."""
    n = rhs.size // 2
    x1 = pcg_fixed(A11, rhs[:n], prec1, k, first_rz_factor)
    x2 = pcg_fixed(A22, rhs[n:] - A21 @ x1, prec2, k)
    return np.concatenate([x1, x2])


def sweep_problem(kind, nx, ny, nz, k1=K1, k2=K2, beta=BETA, mu=MU):
    """Blocks, right-hand side, boundary lift and the two hierarchies of a mesh with the Dirichlet sets of variant 0."""
    dim = dim_of(kind)
    om = o.build_mesh(dim, kind, nx, ny, nz)
    n = om.num_nodes
    nodes = [dirichlet_nodes(kind, nx, ny, nz, 0, f) for f in (0, 1)]
    g = [np.zeros(n), np.zeros(n)]
    for f in (0, 1):
        g[f][nodes[f]] = dirichlet_values(kind, nx, ny, nz, nodes[f], f)
    masks = [mask_of(n, nodes[f]) for f in (0, 1)]
    osys = o.build_system(om, o.Params(k1=k1, k2=k2, beta=beta, mu=mu), g[0], g[1], mms=False, mask1=masks[0], mask2=masks[1])
    A = osys.A.tocsr()
    lv = [G.build_hierarchy(dim, kind, nx, ny, nz, (k1 / mu, k2 / mu)[f], beta / mu, masks[f]) for f in (0, 1)]
    return {"A11": A[:n, :n], "A22": A[n:, n:], "A21": A[n:, :n], "rhs": osys.rhs, "u0": osys.u0, "levels": lv, "n": n,
            "nodes": nodes, "values": [g[f][nodes[f]] for f in (0, 1)]}


def sweep_reference(p, k, first_rz_factor=1.0):
    pre = [lambda v, f=f: apply_reference(p["levels"][f], v, 1) for f in (0, 1)]
    return picard_sweep(p["A11"], p["A22"], p["A21"], p["rhs"], pre[0], pre[1], k, first_rz_factor)


def sweep_drift(p, k, seed=31):
    """Reference against itself with both hierarchies and blocks renumbered at random."""
    n = p["n"]
    pl = [permuted(p["levels"][f], seed + f) for f in (0, 1)]
    pre = [lambda v, f=f: apply_permuted(pl[f][0], pl[f][1], v, 1) for f in (0, 1)]
    du = picard_sweep(p["A11"], p["A22"], p["A21"], p["rhs"], pre[0], pre[1], k)
    return rel_err(du, sweep_reference(p, k))


def sweep_bound(p, k):
    """1e-10 for k = 1 (the cycle's bound); k = 2, 3: 100 x the reference's own drift, at least 1e-13."""
    return CYCLE_BOUND if k == 1 else max(100 * sweep_drift(p, k), 1e-13)


# ---------------------------------------------------------------------------------------------------------------------
# matrix-free hierarchy for uniform quadrilaterals / hexahedra
# ---------------------------------------------------------------------------------------------------------------------
def _p1_tridiagonals(ncell: int):
    """(lo, di, up) of the 1D P1 stiffness and mass matrices on ncell cells of [0, 1]."""
    h = 1.0 / ncell
    p = ncell + 1
    kd = np.full(p, 2.0 / h)
    kd[0] = kd[-1] = 1.0 / h
    ko = np.full(p, -1.0 / h)
    md = np.full(p, 4.0 * h / 6.0)
    md[0] = md[-1] = 2.0 * h / 6.0
    mo = np.full(p, h / 6.0)

    def tri(d, off):
        lo, up = off.copy(), off.copy()
        lo[0] = 0.0
        up[-1] = 0.0
        return lo, d, up

    return tri(kd, ko), tri(md, mo)


_IDENT = None   # the 1 x 1 "mass matrix" of the missing z direction in 2D


def _tri_apply(t, x: np.ndarray, axis: int) -> np.ndarray:
    if t is _IDENT:
        return x
    lo, di, up = t
    sh = [1, 1, 1]
    sh[axis] = -1
    y = di.reshape(sh) * x
    a = [slice(None)] * 3
    b = [slice(None)] * 3
    a[axis], b[axis] = slice(1, None), slice(None, -1)
    y[tuple(a)] += lo[1:].reshape(sh) * x[tuple(b)]
    y[tuple(b)] += up[:-1].reshape(sh) * x[tuple(a)]
    return y


class MatfreeOperator:
    """A_e = elimination of coefK K + coefM M on a uniform (nx, ny[, nz]) Q1 mesh; ``A @ x`` for flat x."""

    def __init__(self, cells, coefK: float, coefM: float, mask: np.ndarray):
        nx, ny, nz = cells
        self.dim = 3 if nz > 0 else 2
        self.shape3 = (nz + 1 if self.dim == 3 else 1, ny + 1, nx + 1)
        self.cK, self.cM = coefK, coefM
        self.mask3 = np.asarray(mask, bool).reshape(self.shape3)
        self.Kx, self.Mx = _p1_tridiagonals(nx)
        self.Ky, self.My = _p1_tridiagonals(ny)
        self.Kz, self.Mz = _p1_tridiagonals(nz) if self.dim == 3 else (None, _IDENT)
        n = self.mask3.size
        self.shape = (n, n)

    def full(self, x3: np.ndarray) -> np.ndarray:
        """(coefK K + coefM M) x = Kx (cK a) + Mx (cK (b + c) + cM a), a = My Mz x, b = Ky Mz x, c = My Kz x."""
        mz = _tri_apply(self.Mz, x3, 0)
        a = _tri_apply(self.My, mz, 1)
        s = _tri_apply(self.Ky, mz, 1)
        if self.dim == 3:
            s = s + _tri_apply(self.My, _tri_apply(self.Kz, x3, 0), 1)
        return _tri_apply(self.Kx, self.cK * a, 2) + _tri_apply(self.Mx, self.cK * s + self.cM * a, 2)

    def __matmul__(self, x: np.ndarray) -> np.ndarray:
        x3 = x.reshape(self.shape3)
        y = self.full(np.where(self.mask3, 0.0, x3))
        y[self.mask3] = x3[self.mask3]
        return y.ravel()

    def _coef(self, dx: int, dy: int, dz: int) -> np.ndarray:
        """Stencil coefficient a(i, i + d) of the full operator at every node (0 where i + d is outside the box)."""
        pick = lambda t, d: (np.ones(1) if t is _IDENT else t[d + 1])   # noqa: E731
        if self.dim == 2 and dz != 0:
            return np.zeros(self.shape3)
        mz, my = pick(self.Mz, dz)[:, None], pick(self.My, dy)[None, :]
        g1 = self.cK * my * mz
        g2 = self.cK * pick(self.Ky, dy)[None, :] * mz + self.cM * my * mz
        if self.dim == 3:
            g2 = g2 + self.cK * my * pick(self.Kz, dz)[:, None]
        return pick(self.Kx, dx)[None, None, :] * g1[:, :, None] + pick(self.Mx, dx)[None, None, :] * g2[:, :, None]

    def diagonal_and_bound(self):
        """(diagonal of A_e, max row sum of |D^-1 A_e|)."""
        free = np.pad(~self.mask3, 1, constant_values=False).astype(np.float64)
        pz, py, px = self.shape3
        rows = np.zeros(self.shape3)
        diag = None
        for dz in ((-1, 0, 1) if self.dim == 3 else (0,)):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    c = self._coef(dx, dy, dz)
                    if (dx, dy, dz) == (0, 0, 0):
                        diag = c.copy()
                    rows += np.abs(c) * free[1 + dz:1 + dz + pz, 1 + dy:1 + dy + py, 1 + dx:1 + dx + px]
        diag[self.mask3] = 1.0
        rows[self.mask3] = 1.0
        return diag.ravel(), float((rows / diag).max())


class AxisTransfer:
    """Multilinear interpolation coarse -> fine as 1D interpolations per axis; ``P @ xc``, ``P.T @ rf``."""

    def __init__(self, cshape3, fshape3, transposed: bool = False):
        self.c, self.f, self.transposed = tuple(cshape3), tuple(fshape3), transposed
        self.shape = (int(np.prod(self.c)), int(np.prod(self.f))) if transposed else (int(np.prod(self.f)), int(np.prod(self.c)))

    @property
    def T(self):
        return AxisTransfer(self.c, self.f, not self.transposed)

    def __matmul__(self, v: np.ndarray) -> np.ndarray:
        if not self.transposed:
            x = v.reshape(self.c)
            for ax in range(3):
                if self.f[ax] == self.c[ax]:
                    continue
                sh = list(x.shape)
                sh[ax] = self.f[ax]
                y = np.empty(sh)
                ev, od, lo, hi = ([slice(None)] * 3 for _ in range(4))
                ev[ax], od[ax], lo[ax], hi[ax] = slice(0, None, 2), slice(1, None, 2), slice(None, -1), slice(1, None)
                y[tuple(ev)] = x
                y[tuple(od)] = 0.5 * (x[tuple(lo)] + x[tuple(hi)])
                x = y
            return x.ravel()
        r = v.reshape(self.f)
        for ax in range(3):
            if self.f[ax] == self.c[ax]:
                continue
            ev, od, lo, hi = ([slice(None)] * 3 for _ in range(4))
            ev[ax], od[ax], lo[ax], hi[ax] = slice(0, None, 2), slice(1, None, 2), slice(None, -1), slice(1, None)
            y = r[tuple(ev)].copy()
            half = 0.5 * r[tuple(od)]
            y[tuple(lo)] += half
            y[tuple(hi)] += half
            r = y
        return r.ravel()


def matfree_hierarchy(kind: int, nx: int, ny: int, nz: int, coefK: float, coefM: float, mask_fine: np.ndarray):
    """``dpp_mg_oracle.build_hierarchy`` for QUAD / HEX without matrices (same Level fields, A and P as operators)."""
    assert kind in (QUAD, HEX)
    cells = level_cells(kind, nx, ny, nz)
    mask = np.asarray(mask_fine, bool)
    levels = []
    for l, c in enumerate(cells):
        A = MatfreeOperator(c, coefK, coefM, mask)
        d, lam = A.diagonal_and_bound()
        levels.append(G.Level(A, 1.0 / d, mask.copy(), lam))
        if l > 0:
            levels[l - 1].P = AxisTransfer(A.shape3, levels[l - 1].A.shape3)
        if l + 1 < len(cells):
            m3 = A.mask3
            mask = (m3[::2, ::2, ::2] if A.dim == 3 else m3[:, ::2, ::2]).ravel().copy()
    return levels
