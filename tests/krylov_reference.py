"""The monolithic Krylov loops of perphil_amd/csrc/pph_solve.hip (cg_solve with norm_type 0, gmres_solve) restated in NumPy, in
any float type, for tests/test_krylov_scale_host.py and tests/test_krylov_scale_gpu.py.

The loops are written from the conventions of pph_solve.hip, statement for statement, not from the oracle's ``pcg`` / ``gmres``
(modified Gram-Schmidt there, classical here; the oracle divides by the norms, the device multiplies by their reciprocals).
Every vector operation goes through an ``Ops`` object whose methods are the BLAS-1 kernels of pph_la.hip - k_mdot, k_dot2,
k_maxpy, k_cg_update, k_axpby - so that the host file can run each loop with ONE of them leaving out the rows of its last
grid-stride pass (the mutants) and show that the comparison of the GPU file would notice.

The operator is a callable; the systems of asm_scale_reference (``System.apply("MONO", .)``) are products without a matrix, so a
loop on a million rows costs a second or two.  Preconditioners are vectors: ``jacobi_vector``, ``block2_vectors``.
``perturbed`` is the same system with every product multiplied row by row by 1 + 4 eps xi: it stands for the device's other
summation order and for its own rounding of the assembled entries.  ``reference`` runs a loop in fp64, perturbed fp64 and
longdouble - the latter on the fp64 box matrices and, as ``LongdoubleSystem``, with the box matrices in longdouble too - and returns
the fp64 result with the reference-only discrepancies (delta_hist, delta_x; delta_loop) the GPU file's bounds are multiples of.

The last part restates the launch rules of pph_la.hip (ew_grid, RED_BLOCKS, spmv_grid) and of k_block2_build / k_block2, as
asm_scale_reference restates those of the assembly."""
from __future__ import annotations

import math
import os
import sys
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import asm_scale_reference as R  # noqa: E402
import transient_reference as T  # noqa: E402

EPS = 2.0 ** -52
FACTOR = 100.0       # the rule of tests/README.md for the norms: max(100 delta, 1e-13)
FLOOR = 1e-13


# ---------------------------------------------------------------------------------------------------------------------
# the vector kernels
# ---------------------------------------------------------------------------------------------------------------------
class Ops:
    """The BLAS-1 kernels the loops run on.  A mutant overrides one method."""

    def dot(self, a, b):
        """k_mdot<1> as la_mdot_seg(V, 0, 1, V) uses it for the norms."""
        return np.dot(a, b)

    def spmv_dot(self, p, q):
        """The fused p.Ap of k_spmv_wide<., DOT>."""
        return np.dot(p, q)

    def mdot(self, V, w):
        """k_mdot<4|2|1>: V_i . w for the k + 1 basis vectors."""
        return [np.dot(v, w) for v in V]

    def dot2(self, r, z):
        """k_dot2: (r.z, z.z)."""
        return np.dot(r, z), np.dot(z, z)

    def maxpy(self, w, V, h, sign):
        """k_maxpy: w += sign * sum_q h[q] V_q, the sum formed first (from 0, in the order of q)."""
        s = np.zeros_like(w)
        for hq, v in zip(h, V):
            s += hq * v
        w += sign * s

    def cg_update(self, x, r, p, q, alpha, dinv):
        """k_cg_update: x += alpha p ; r -= alpha q ; z = dinv .* r ; (r.z, z.z).  Returns (z, r.z, z.z)."""
        x += alpha * p
        r -= alpha * q
        z = dinv * r if dinv is not None else r.copy()
        return z, np.dot(r, z), np.dot(z, z)

    def axpy(self, y, a, x):
        y += a * x

    def axpby(self, p, z, beta):
        """k_axpby with a = 1: p = z + beta p."""
        p *= beta
        p += z


class KspOut:
    def __init__(self, x, hist, its, converged, breakdown):
        self.x, self.hist, self.iterations, self.converged, self.breakdown = x, np.array(hist, dtype=x.dtype), its, converged, breakdown


def _is_nan(v) -> bool:
    return not (v == v)


# ---------------------------------------------------------------------------------------------------------------------
# cg_solve, norm_type 0 (the preconditioned norm)
# ---------------------------------------------------------------------------------------------------------------------
def pcg(apply_A: Callable, b, apply_pc, max_it: int, rtol: float, atol: float, dtype=np.float64, ops: Optional[Ops] = None) -> KspOut:
    """apply_pc: None (z = r through the fused update), a VECTOR (point Jacobi: the fused k_cg_update) or a callable (the
    unfused branch: axpy, axpy, pc, k_dot2).  hist[k] = sqrt(z_k . z_k); tolerance max(rtol hist[0], atol); breakdown
    !(p.Ap > 0)."""
    ops = ops or Ops()
    b = np.asarray(b).astype(dtype)
    fused = apply_pc is None or not callable(apply_pc)
    dinv = None if apply_pc is None or callable(apply_pc) else np.asarray(apply_pc).astype(dtype)
    x = np.zeros_like(b)
    r = b.copy()
    z = (dinv * r if dinv is not None else r.copy()) if fused else apply_pc(r)
    rz, zz = ops.dot2(r, z)
    res = np.sqrt(zz)
    tol = max(dtype(rtol) * res, dtype(atol))
    hist = [res]
    if _is_nan(res):
        return KspOut(x, hist, 0, False, True)
    if res <= tol:
        return KspOut(x, hist, 0, True, False)
    p = z.copy()
    its, converged, breakdown = 0, False, False
    while its < max_it:
        q = apply_A(p)
        pq = ops.spmv_dot(p, q)
        if not (pq > 0) or _is_nan(rz):
            breakdown = True
            break
        alpha = rz / pq
        if fused:
            z, rz_new, zz = ops.cg_update(x, r, p, q, alpha, dinv)
        else:
            ops.axpy(x, alpha, p)
            ops.axpy(r, -alpha, q)
            z = apply_pc(r)
            rz_new, zz = ops.dot2(r, z)
        res = np.sqrt(zz)
        its += 1
        hist.append(res)
        if _is_nan(res):
            breakdown = True
            break
        if res <= tol:
            converged = True
            break
        ops.axpby(p, z, rz_new / rz)
        rz = rz_new
    return KspOut(x, hist, its, converged, breakdown)


# ---------------------------------------------------------------------------------------------------------------------
# gmres_solve
# ---------------------------------------------------------------------------------------------------------------------
def gmres_left(apply_A: Callable, b, apply_pc, restart: int, max_it: int, rtol: float, atol: float, dtype=np.float64,
               ops: Optional[Ops] = None) -> KspOut:
    """Left-preconditioned restarted GMRES: classical Gram-Schmidt in one pass (one multi-dot, one multi-axpy), Givens
    recurrence, hist[k] = |g[k + 1]|; a cycle cut short by max_it updates with the columns built so far; the restart residual is
    P^-1 (b - A x); convergence is res <= tol.  apply_pc: None, a vector or a callable."""
    ops = ops or Ops()
    b = np.asarray(b).astype(dtype)
    if apply_pc is None:
        pc = lambda v: v.copy()   # noqa: E731
    elif callable(apply_pc):
        pc = apply_pc
    else:
        dv = np.asarray(apply_pc).astype(dtype)
        pc = lambda v: dv * v     # noqa: E731
    one = dtype(1)
    x = np.zeros_like(b)
    v0 = pc(b)
    beta = np.sqrt(ops.dot(v0, v0))
    tol = max(dtype(rtol) * beta, dtype(atol))
    hist = [beta]
    if _is_nan(beta):
        return KspOut(x, hist, 0, False, True)
    if beta <= tol:
        return KspOut(x, hist, 0, True, False)
    its, res, first, breakdown = 0, beta, True, False
    while its < max_it:
        if not first:
            v0 = pc(b - apply_A(x))
            beta = np.sqrt(ops.dot(v0, v0))
        first = False
        V = [v0 * (one / beta)]
        H = np.zeros((restart + 1, restart), dtype)
        cs, sn, g = np.zeros(restart, dtype), np.zeros(restart, dtype), np.zeros(restart + 1, dtype)
        g[0] = beta
        kused, done = 0, False
        for k in range(restart):
            w = pc(apply_A(V[k]))
            h = ops.mdot(V[:k + 1], w)
            ops.maxpy(w, V[:k + 1], h, -one)
            hn = np.sqrt(ops.dot(w, w))
            H[:k + 1, k] = h
            H[k + 1, k] = hn
            V.append(w * (one / hn) if hn > 0 else np.zeros_like(w))
            for i in range(k):
                t = cs[i] * H[i, k] + sn[i] * H[i + 1, k]
                H[i + 1, k] = -sn[i] * H[i, k] + cs[i] * H[i + 1, k]
                H[i, k] = t
            d = np.hypot(H[k, k], H[k + 1, k])
            if not (d > 0):
                breakdown, done, kused = True, True, k
                break
            cs[k], sn[k] = H[k, k] / d, H[k + 1, k] / d
            H[k, k], H[k + 1, k] = d, 0
            g[k + 1] = -sn[k] * g[k]
            g[k] = cs[k] * g[k]
            its += 1
            kused = k + 1
            res = abs(g[k + 1])
            hist.append(res)
            if res <= tol or its >= max_it:
                done = True
                break
        y = np.zeros(restart, dtype)
        for i in range(kused - 1, -1, -1):
            s = g[i]
            for j in range(i + 1, kused):
                s -= H[i, j] * y[j]
            y[i] = s / H[i, i]
        if kused > 0:
            ops.maxpy(x, V[:kused], y[:kused], one)
        if done:
            break
    return KspOut(x, hist, its, bool(res <= tol) and not breakdown, breakdown)


# ---------------------------------------------------------------------------------------------------------------------
# preconditioners as vectors, on asm_scale_reference.System
# ---------------------------------------------------------------------------------------------------------------------
def jacobi_vector(S) -> np.ndarray:
    """1 / diag of the monolithic system (k_diag_inv); the constrained rows are unit rows: 1."""
    return 1.0 / np.concatenate([S.diag(0), S.diag(1)])


def block2_vectors(S) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The inverse of the 2 x 2 block of every node as k_block2_build forms it: d11, d22 from the diagonals of the diagonal
    blocks, d12 = d21 from the diagonal of the coupling (-beta / mu diag(M) where both fields are free, 0 elsewhere)."""
    both = ~S.masks[0] & ~S.masks[1]
    d12 = np.where(both, -R.diagonal(S.kind, S.nd, 0.0, S.b), 0.0)
    return block2_from_diagonals(S.diag(0), S.diag(1), d12, d12)


def block2_from_diagonals(d11, d22, d12, d21) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """k_block2_build: r = 1 / det ; (d22 r, -d12 r, -d21 r, d11 r); the identity where the determinant is 0."""
    det = d11 * d22 - d12 * d21
    ok = det != 0.0
    r = 1.0 / np.where(ok, det, 1.0)
    return (np.where(ok, d22 * r, 1.0), np.where(ok, -d12 * r, 0.0), np.where(ok, -d21 * r, 0.0), np.where(ok, d11 * r, 1.0))


def block2_apply(binv: Sequence[np.ndarray], dtype=np.float64, skip: Optional[np.ndarray] = None) -> Callable:
    """k_block2: z1 = b11 r1 + b12 r2 ; z2 = b21 r1 + b22 r2 per node.  ``skip`` (a mutant): nodes the kernel never reaches -
    their z keeps what the buffer held before (zeros at first)."""
    b11, b12, b21, b22 = (np.asarray(q).astype(dtype) for q in binv)
    n = b11.size
    state = {"z": np.zeros(2 * n, dtype)}

    def apply(r):
        z = np.concatenate([b11 * r[:n] + b12 * r[n:], b21 * r[:n] + b22 * r[n:]])
        if skip is not None:
            both = np.concatenate([skip, skip])
            z[both] = state["z"][both]
            state["z"] = z.copy()
        return z
    return apply


def box_matrices_longdouble(kind: int, nd) -> Tuple[np.ndarray, np.ndarray]:
    """transient_reference.box_matrices, the same closed form, with every operation in longdouble: the thirds, sixths and
    ninths of the box matrices to 1e-19 instead of fp64's 1e-16."""
    ld = np.longdouble
    dim = len(nd)
    nc = 1 << dim
    vol = ld(1) / ld(math.prod(int(q) for q in nd))
    KB, MB = np.zeros((nc, nc), ld), np.zeros((nc, nc), ld)
    if kind in (R.QUAD, R.HEX):
        S = np.array([[1, -1], [-1, 1]], dtype=ld)
        Mm = np.array([[2, 1], [1, 2]], dtype=ld) / ld(6)
        for a in range(nc):
            for b in range(nc):
                ab = [((a >> e) & 1, (b >> e) & 1) for e in range(dim)]
                m, k = ld(1), ld(0)
                for i, j in ab:
                    m = m * Mm[i, j]
                for d in range(dim):
                    t = ld(int(nd[d]) ** 2)
                    for e in range(dim):
                        t = t * (S if e == d else Mm)[ab[e]]
                    k = k + t
                MB[a, b], KB[a, b] = vol * m, vol * k
        return KB, MB
    subs = T._SUBCELLS[kind]
    vc = vol / ld(len(subs))
    for v in subs:
        for d in range(dim):
            lo, up = [(q, t) for q in range(dim + 1) for t in range(dim + 1) if v[t] == (v[q] | (1 << d)) and v[t] != v[q]][0]
            e = np.zeros(dim + 1, ld)
            e[up], e[lo] = 1, -1
            for r in range(dim + 1):
                for s in range(dim + 1):
                    KB[v[r], v[s]] += vc * ld(int(nd[d]) ** 2) * e[r] * e[s]
        for r in range(dim + 1):
            for s in range(dim + 1):
                MB[v[r], v[s]] += vc * ld(2 if r == s else 1) / ld((dim + 1) * (dim + 2))
    return KB, MB


class LongdoubleSystem(R.System):
    """asm_scale_reference.System in longdouble THROUGHOUT.  System(dtype=longdouble) adds and multiplies in longdouble but reads
    the box matrices that transient_reference.box_matrices rounded to fp64, so its operator is to the last bit the fp64 run's:
    the two differ by the rounding of sums and products only, and nothing of the distance between an fp64 REPRESENTATION of the
    operator and the operator.  Here the box matrices are longdouble too (box_matrices_longdouble); the coefficients a, b, c are
    the fp64 numbers the device is given.  The fp64 run against this one holds what any fp64 form of the operator - box matrices
    rounded per entry there, assembled entries rounded per entry on the device - is away from the exact one: half an ulp per
    entry, the SAME in every product of a loop and relative to |A| |x|, which a stiffness row cancels by 1 / h^2 on the smooth
    part of a vector."""

    def __init__(self, kind, nd, cf, sigma, masks, g):
        super().__init__(kind, nd, cf, sigma, masks, g, np.longdouble)
        self._boxes = box_matrices_longdouble(kind, list(nd))

    def _ba(self, cK, cM, x, absolute):
        ld = np.longdouble
        KB, MB = self._boxes
        W = abs(ld(cK) * KB) + abs(ld(cM) * MB) if absolute else ld(cK) * KB + ld(cM) * MB
        X = np.asarray(x).astype(ld).reshape(R.shape_of(self.nd))
        return R.gather(W, abs(X) if absolute else X).ravel()


class perturbed:
    """The same system whose every product is multiplied row by row by 1 + 4 eps xi, xi seeded uniform in [-1, 1]."""

    def __init__(self, system, seed: int):
        self._s, self._rng = system, np.random.default_rng(seed)

    def __getattr__(self, name):
        return getattr(self._s, name)

    def apply(self, which, x, absolute=False):
        y = self._s.apply(which, x, absolute)
        return y * (1.0 + 4.0 * EPS * self._rng.uniform(-1.0, 1.0, y.size)).astype(y.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# launch rules of pph_la.hip and of the block-2 kernels of pph_solve.hip, restated
# ---------------------------------------------------------------------------------------------------------------------
BLOCK = 256
EW_MAX_WG = 2048          # ew_grid
RED_BLOCKS = 1024         # grid of the reductions
SPMV_DEF_BLOCKS, SPMV_MAX_BLOCKS = 1024, 2048
BLOCK2_BUILD_MAX_WG = 2048
MDOT_WIDTHS = (4, 2, 1)


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _passes(items: int, grid: int) -> Tuple[int, int]:
    stride = grid * BLOCK
    passes = _cdiv(items, stride)
    return passes, items - (passes - 1) * stride


def la_launch(N: int) -> Dict[str, int]:
    """The element-wise kernels over N entries (ew_grid: min(ceil(N / 512), 2048) workgroups of 256 threads) and the reductions
    (the same grid cut to RED_BLOCKS; k_reduce_final then adds `partials` sums per slot).  `last`: rows of the last pass."""
    grid = max(1, min(_cdiv(N, 2 * BLOCK), EW_MAX_WG))
    passes, last = _passes(N, grid)
    rgrid = min(grid, RED_BLOCKS)
    rpasses, rlast = _passes(N, rgrid)
    return {"grid": grid, "passes": passes, "last": last, "red_grid": rgrid, "red_passes": rpasses, "red_last": rlast, "partials": rgrid}


def block2_launch(n: int) -> Dict[str, int]:
    """k_block2_build: one node per thread on at most 2048 workgroups; k_block2 (and the per-field passes): ew_grid(n)."""
    bgrid = max(1, min(_cdiv(n, BLOCK), BLOCK2_BUILD_MAX_WG))
    bpasses, blast = _passes(n, bgrid)
    L = la_launch(n)
    return {"build_grid": bgrid, "build_passes": bpasses, "build_last": blast, "grid": L["grid"], "passes": L["passes"], "last": L["last"]}


def spmv_launch(N: int, max_row: int, lanes: int = 0, blocks: int = 0) -> Dict[str, int]:
    """k_spmv_wide<G, .> on the monolithic CSR: G lanes per row (4 for rows of up to 13 entries, else 8; option spmv_lanes),
    256 / G rows per chunk, grid = min(chunks, cap) rounded up to a multiple of 8, cap = 1024 or option spmv_blocks; a row takes
    `steps` aligned 4-wide steps of its G lanes (one more where it starts off a multiple of 4)."""
    G = lanes if lanes in (4, 8, 16, 32, 64) else (4 if 0 < max_row and max_row + 3 <= 16 else 8)
    cap = (blocks // 8) * 8 if 8 <= blocks <= SPMV_MAX_BLOCKS else SPMV_DEF_BLOCKS
    chunks = _cdiv(N, BLOCK // G)
    grid = _cdiv(min(chunks, cap), 8) * 8
    return {"lanes": G, "chunks": chunks, "grid": grid, "passes": _cdiv(chunks, grid), "steps": _cdiv(max_row + 3, 4 * G), "partials": grid}


def mdot_widths(k: int) -> Tuple[int, ...]:
    """The launches la_mdot_seg splits k dot products into."""
    out = []
    while k > 0:
        w = 4 if k >= 4 else 2 if k >= 2 else 1
        out.append(w)
        k -= w
    return tuple(out)


def tail_mask(N: int, last: int) -> np.ndarray:
    m = np.zeros(N, dtype=bool)
    m[N - last:] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the GPU file
# ---------------------------------------------------------------------------------------------------------------------
LARGE = {"quad1024x512": (R.QUAD, (1024, 512)), "quad2048x512": (R.QUAD, (2048, 512)), "hex128x64x64": (R.HEX, (128, 64, 64))}
# (ksp, pc, restart, max_it) per mesh
LOOPS = {
    "quad1024x512": [("gmres", pc, 7, 10) for pc in ("none", "jacobi", "block2")] + [("cg", pc, 0, 6) for pc in ("none", "jacobi", "block2")],
    "quad2048x512": [("cg", "block2", 0, 3), ("gmres", "block2", 3, 4)],
    "hex128x64x64": [("cg", "jacobi", 0, 3)],
}
B_SEED = 5
PERT_SEED = 9

_setup_cache: Dict[tuple, dict] = {}
_ref_cache: Dict[tuple, dict] = {}


def clear() -> None:
    _setup_cache.clear()
    _ref_cache.clear()
    R.clear_pieces()


def setup(kind: int, nd: Sequence[int], constrain_all: bool = False) -> dict:
    """Mesh, Dirichlet sets and data of asm_scale_reference (CF, unshifted), b seeded uniform in [0.5, 1.5] (the device masks
    it: b is 0 on the constrained rows here).  constrain_all: every node in both sets.  One mesh at a time is kept."""
    key = (kind, tuple(nd), bool(constrain_all))
    if key not in _setup_cache:
        _setup_cache.clear()      # (the references of earlier meshes stay: an iterate and a history each)
        R.clear_pieces()
        n = R.num_nodes(nd)
        nodes = (np.arange(n), np.arange(n)) if constrain_all else R.dirichlet_sets(kind, nd)
        masks = T.masks_of(n, *nodes)
        g = R.dirichlet_data(n, nodes)
        free = ~np.concatenate(masks)
        b_full = np.random.default_rng(B_SEED).uniform(0.5, 1.5, 2 * n)
        _setup_cache[key] = {"kind": kind, "nd": tuple(nd), "n": n, "nodes": nodes, "masks": masks, "g": g, "free": free,
                             "b_full": b_full, "b": np.where(free, b_full, 0.0)}
    return _setup_cache[key]


def system(c: dict, dtype=np.float64):
    return R.System(c["kind"], c["nd"], R.CF, (0.0, 0.0), c["masks"], c["g"], dtype)


def preconditioner(S, pc: str, dtype=np.float64, skip=None):
    if pc == "none":
        return None
    if pc == "jacobi":
        return jacobi_vector(S).astype(dtype)
    assert pc == "block2"
    return block2_apply(block2_vectors(S), dtype, skip)


def run(c: dict, ksp: str, pc: str, restart: int, max_it: int, rtol: float = 0.0, atol: float = 0.0, dtype=np.float64,
        pert: bool = False, ops: Optional[Ops] = None, skip=None, b=None, exact_boxes: bool = False) -> KspOut:
    """exact_boxes (longdouble only): the products of LongdoubleSystem; the preconditioner VECTORS stay those of the fp64
    system, cast: they are part of the loop's statement, and an eps in them is an eps in z, not in A."""
    S = system(c, dtype)
    P = preconditioner(S, pc, dtype, skip)
    if exact_boxes:
        assert dtype is np.longdouble and not pert
        S = LongdoubleSystem(c["kind"], c["nd"], R.CF, (0.0, 0.0), c["masks"], c["g"])
    if pert:
        S = perturbed(S, PERT_SEED)
    A = lambda v: S.apply("MONO", v)   # noqa: E731
    b = c["b"] if b is None else b
    if ksp == "cg":
        return pcg(A, b, P, max_it, rtol, atol, dtype, ops)
    return gmres_left(A, b, P, restart, max_it, rtol, atol, dtype, ops)


def run_on_matrix(A, b, ksp: str, pc: str, restart: int, max_it: int, rtol: float = 0.0, atol: float = 0.0) -> KspOut:
    """The same loops in fp64 on an ASSEMBLED matrix (scipy CSR, field-major 2n x 2n), with the preconditioner vectors taken
    from its own diagonals as k_diag_inv and k_block2_build take them."""
    n = A.shape[0] // 2
    if pc == "none":
        P = None
    elif pc == "jacobi":
        d = A.diagonal()
        P = 1.0 / np.where(d != 0.0, d, 1.0)
    else:
        P = block2_apply(block2_from_diagonals(A[:n, :n].diagonal(), A[n:, n:].diagonal(), A[:n, n:].diagonal(), A[n:, :n].diagonal()))
    op = lambda v: A @ v   # noqa: E731
    if ksp == "cg":
        return pcg(op, b, P, max_it, rtol, atol)
    return gmres_left(op, b, P, restart, max_it, rtol, atol)


def hist_distance(h, href) -> float:
    """max_k |h_k - href_k| / |href_k| (entries that are 0 in both agree; lengths must agree)."""
    h, href = np.asarray(h, dtype=np.longdouble), np.asarray(href, dtype=np.longdouble)
    if h.shape != href.shape:
        return float("inf")
    d = abs(h - href)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(href != 0, d / np.where(href != 0, abs(href), 1), np.where(d > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


def x_distance(x, xref) -> float:
    """max |dx| / max |xref|."""
    x, xref = np.asarray(x, dtype=np.longdouble), np.asarray(xref, dtype=np.longdouble)
    m = abs(xref).max()
    d = abs(x - xref).max()
    return float(d / m) if m > 0 else (0.0 if d == 0 else float("inf"))


def bars(delta_hist: float, delta_x: float) -> Tuple[float, float]:
    return max(FACTOR * delta_hist, FLOOR), max(FACTOR * delta_x, FLOOR)


def reference(c: dict, ksp: str, pc: str, restart: int, max_it: int, rtol: float = 0.0, atol: float = 0.0) -> dict:
    """The fp64 restatement of a loop with its reference-only discrepancies: against its longdouble run and against its
    perturbed run; delta = the larger.  Cached per (mesh, loop) and never changed afterwards.

    The longdouble run is made twice.  On the fp64-rounded box matrices (System(dtype=longdouble)) it differs from the fp64 run by
    the rounding of the loop's sums and products alone: with the perturbed run that is delta_loop / bars_loop, the bar of a
    comparison in which both sides hold the SAME stored operator (the GPU file's device-matrix variants).  In longdouble
    throughout (LongdoubleSystem) it also holds what the fp64 form of the operator itself is away from the operator: with the
    other two that is delta / bars, the bar against the matrix-free restatement, whose operator and the device's are two
    different fp64 roundings of one operator."""
    key = (c["kind"], c["nd"], bool(c["free"].any()), ksp, pc, restart, max_it, rtol, atol)
    if key not in _ref_cache:
        f64 = run(c, ksp, pc, restart, max_it, rtol, atol)
        per = run(c, ksp, pc, restart, max_it, rtol, atol, pert=True)
        ld = run(c, ksp, pc, restart, max_it, rtol, atol, dtype=np.longdouble)
        ldx = run(c, ksp, pc, restart, max_it, rtol, atol, dtype=np.longdouble, exact_boxes=True)
        dh_loop = max(hist_distance(f64.hist, ld.hist), hist_distance(f64.hist, per.hist))
        dx_loop = max(x_distance(f64.x, ld.x), x_distance(f64.x, per.x))
        dh, dx = max(dh_loop, hist_distance(f64.hist, ldx.hist)), max(dx_loop, x_distance(f64.x, ldx.x))
        f64.x.setflags(write=False)
        f64.hist.setflags(write=False)
        _ref_cache[key] = {"out": f64, "x": f64.x, "hist": f64.hist, "delta_hist": dh, "delta_x": dx, "bars": bars(dh, dx),
                           "delta_loop": (dh_loop, dx_loop), "bars_loop": bars(dh_loop, dx_loop),
                           "same_count": f64.iterations == per.iterations == ld.iterations == ldx.iterations}
    return _ref_cache[key]
