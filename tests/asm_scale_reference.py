"""Matrix-free fp64 reference for the CG-1 assembly and the step kernels at sizes past their launch caps, for
tests/test_asm_scale_host.py and tests/test_asm_scale_gpu.py.

Everything here is built on ONE product, ``box_apply``: (coefK K + coefM M) x on the uniform mesh as a gather over box
corners.  For every corner pair (a, b) of ``transient_reference.box_matrices`` the nodes that are corner a of an existing
box receive W[a, b] times the value at that box's corner b; with the node array reshaped to (pz, py, px) both node sets are
slices.  No matrix is built and no dof map is read, so a mesh of four million nodes costs about a second per product.

On top of it: the un-eliminated operator with a shift per field, the Dirichlet-eliminated blocks as products (the convention
of ``transient_reference.shifted_blocks``), the lifted right-hand side, ``step_rhs`` and the diagonal (3^d coloured impulses).
``absolute=True`` gives the row-wise magnitude (|coefK KB| + |coefM MB|) |x| that the bounds of the GPU file are multiples of.

The second half restates the launch rules of perphil_amd/csrc/pph_assemble.hip (pph_launch_fused_kernels) and
pph_transient.hip, as ``post_reference.norm_launch`` does for the norms: which kernel family a context takes and how many
passes a workgroup makes.  Every GPU case asserts from these which side of its threshold it is on.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import dpp_oracle as o  # noqa: E402
import transient_reference as T  # noqa: E402

QUAD, TRI, HEX, TET = o.CELL_QUAD, o.CELL_TRI, o.CELL_HEX, o.CELL_TET
NAMES = {QUAD: "quad", TRI: "tri", HEX: "hex", TET: "tet"}
EPS = T.EPS
BAR = 1e3 * EPS          # the project's bar for the step right-hand side (tests/test_transient_gpu.py), row by row
WHICH = ("A11", "A22", "A12", "A21", "MONO")
CF = T.Coefs(1.3, 0.02, 3.0, 2.0)   # CF of tests/test_transient_gpu.py
# the small ragged meshes of the host file (one and two cells per direction included)
SMALL = [(QUAD, (5, 3)), (TRI, (4, 3)), (HEX, (5, 3, 4)), (TET, (3, 4, 2)), (QUAD, (1, 2)), (TRI, (2, 1)), (HEX, (1, 2, 1)), (TET, (2, 1, 1))]


def dim_of(kind: int) -> int:
    return 2 if kind in (QUAD, TRI) else 3


def num_nodes(nd: Sequence[int]) -> int:
    return int(np.prod([q + 1 for q in nd]))


def shape_of(nd: Sequence[int]) -> Tuple[int, ...]:
    """(pz, py, px) or (py, px)."""
    return tuple(q + 1 for q in reversed(nd))


def node_ijk(nd: Sequence[int]):
    px, py = nd[0] + 1, nd[1] + 1
    idx = np.arange(num_nodes(nd))
    return idx % px, (idx // px) % py, idx // (px * py)


# ---------------------------------------------------------------------------------------------------------------------
# the product
# ---------------------------------------------------------------------------------------------------------------------
def box_apply(kind: int, nd: Sequence[int], coefK: float, coefM: float, x: np.ndarray, absolute: bool = False, dtype=np.float64) -> np.ndarray:
    """(coefK K + coefM M) x; ``absolute``: (|coefK KB| + |coefM MB|) |x|."""
    nd = list(nd)
    dim = len(nd)
    KB, MB = T.box_matrices(kind, nd)
    if absolute:
        W = abs(dtype(coefK) * KB.astype(dtype)) + abs(dtype(coefM) * MB.astype(dtype))
    else:
        W = dtype(coefK) * KB.astype(dtype) + dtype(coefM) * MB.astype(dtype)
    X = np.asarray(x).astype(dtype).reshape(shape_of(nd))
    if absolute:
        X = abs(X)
    return gather(W, X).ravel()


def gather(W: np.ndarray, X: np.ndarray) -> np.ndarray:
    """Y[nodes that are corner a of an existing box] += W[a, b] X[their corner b] for every corner pair; X shaped (pz, py, px)."""
    dim = X.ndim
    Y = np.zeros_like(X)
    for a in range(1 << dim):      # _corner(c): the nodes that are corner c of an existing box (NumPy axes run z, y, x)
        for b in range(1 << dim):
            if W[a, b] != 0:
                Y[_corner(a, dim)] += W[a, b] * X[_corner(b, dim)]
    return Y


def stiffness_term_magnitudes(kind: int, nd: Sequence[int]) -> np.ndarray:
    """Q1 cells: sum_d |box| n_d^2 |S along d x Mm along the others| [a][b], the magnitude of the directional TERMS of
    KB[a][b] before they are added.  |KB| can be far below it - on 128 x 64 x 64 cells (nx^2 = 2 ny^2 + 2 nz^2) the terms of
    the corner pairs that differ in y and z cancel to KB = 0 exactly - and any fp64 evaluation of such an entry carries a
    rounding of the size of its terms: the part of the rounding that the row magnitude of ``box_apply(absolute=True)`` cannot
    see (tests/README_asm_scale.md, "what the comparisons cannot see")."""
    assert kind in (QUAD, HEX)
    dim = len(nd)
    nc = 1 << dim
    vol = 1.0 / float(np.prod(nd))
    S = np.array([[1.0, 1.0], [1.0, 1.0]])
    Mm = np.array([[2.0, 1.0], [1.0, 2.0]]) / 6.0
    KT = np.zeros((nc, nc))
    for a in range(nc):
        for b in range(nc):
            ab = [((a >> e) & 1, (b >> e) & 1) for e in range(dim)]
            KT[a, b] = vol * sum(nd[d] ** 2 * np.prod([(S if e == d else Mm)[ab[e]] for e in range(dim)]) for d in range(dim))
    return KT


def _corner(c: int, dim: int):
    return tuple(slice(1, None) if (c >> e) & 1 else slice(0, -1) for e in reversed(range(dim)))


def diagonal_by_colouring(kind: int, nd: Sequence[int], coefK: float, coefM: float, absolute: bool = False) -> np.ndarray:
    """diag(coefK K + coefM M) by products alone: impulses of one colour of the 3^d colouring are at least three nodes apart,
    so that the product at a node of that colour is its own diagonal entry.  3^d products: for the small meshes."""
    i, j, k = node_ijk(nd)
    dim = len(nd)
    col = (i % 3) + 3 * (j % 3) + (9 * (k % 3) if dim == 3 else 0)
    d = np.zeros(num_nodes(nd))
    for c in range(3 ** dim):
        e = (col == c).astype(np.float64)
        d += e * box_apply(kind, nd, coefK, coefM, e, absolute)
    return d


def diagonal(kind: int, nd: Sequence[int], coefK: float, coefM: float, absolute: bool = False) -> np.ndarray:
    """The same diagonal as the gather would form it for an impulse: W[a, a] summed over the corners a whose box exists (the
    large meshes: 2^d slice additions instead of 3^d products; the host file holds the two against each other)."""
    nd = list(nd)
    dim = len(nd)
    KB, MB = T.box_matrices(kind, nd)
    W = abs(coefK * KB) + abs(coefM * MB) if absolute else coefK * KB + coefM * MB
    Y = np.zeros(shape_of(nd))
    for a in range(1 << dim):
        Y[_corner(a, dim)] += W[a, a]
    return Y.ravel()


# K x, M x (or |KB| |x|, |MB| |x|) of recently seen vectors: every operator of a case is a combination of these, so that the
# option sets and shifts of one mesh share them.  Keyed by the vector's bytes; cleared by the GPU file between meshes.
_PIECES: Dict[tuple, Tuple[np.ndarray, np.ndarray]] = {}
PIECES_MAX = 32


def clear_pieces() -> None:
    _PIECES.clear()


def pieces(kind: int, nd: Sequence[int], x: np.ndarray, absolute: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    x = np.ascontiguousarray(x, dtype=np.float64)
    key = (kind, tuple(nd), bool(absolute), hash(x.tobytes()))
    if key not in _PIECES:
        if len(_PIECES) >= PIECES_MAX:
            _PIECES.pop(next(iter(_PIECES)))
        _PIECES[key] = (box_apply(kind, nd, 1.0, 0.0, x, absolute), box_apply(kind, nd, 0.0, 1.0, x, absolute))
    return _PIECES[key]


class System:
    """The shifted DPP system on a uniform mesh as products: coefficients cf (transient_reference.Coefs), shift sigma per field,
    Dirichlet masks (m0, m1) and values (g0, g1; read on the constrained nodes only)."""

    def __init__(self, kind, nd, cf, sigma, masks, g, dtype=np.float64):
        self.kind, self.nd, self.cf, self.sigma, self.dtype = kind, list(nd), cf, tuple(sigma), dtype
        self.n = num_nodes(nd)
        self.masks = (np.asarray(masks[0], bool), np.asarray(masks[1], bool))
        self.free = tuple((~m).astype(dtype) for m in self.masks)
        self.g = g
        a, b, c = cf.abc
        self.cK = (a, c)
        self.cM = (b + self.sigma[0], b + self.sigma[1])
        self.b = b

    def _ba(self, cK, cM, x, absolute):
        """(cK K + cM M) x.  fp64: combined from the shared pieces K x and M x - a rounding per term more than box_apply's own
        combination, still a few eps of the row magnitude (the host file measures both); longdouble: box_apply itself."""
        if self.dtype is not np.float64:
            return box_apply(self.kind, self.nd, cK, cM, x, absolute, self.dtype)
        kx, mx = pieces(self.kind, self.nd, x, absolute)
        return abs(cK) * kx + abs(cM) * mx if absolute else cK * kx + cM * mx

    # un-eliminated, shifted: [[a K + (b + s1) M, -b M], [-b M, c K + (b + s2) M]]
    def unel(self, p, absolute=False, sigma=None):
        n = self.n
        s = self.sigma if sigma is None else sigma
        sign = 1.0 if absolute else -1.0
        y1 = self._ba(self.cK[0], self.b + s[0], p[:n], absolute) + sign * self._ba(0.0, self.b, p[n:], absolute)
        y2 = self._ba(self.cK[1], self.b + s[1], p[n:], absolute) + sign * self._ba(0.0, self.b, p[:n], absolute)
        return np.concatenate([y1, y2])

    # eliminated blocks: A_ff x = F_f (cK_f K + cM_f M)(F_f x) + (I - F_f) x;  A_fg x = -b F_f M (F_g x)
    def diag_block(self, f, x, absolute=False):
        F = self.free[f]
        x = np.asarray(x).astype(self.dtype)
        if absolute:
            x = abs(x)
        return F * self._ba(self.cK[f], self.cM[f], F * x, absolute) + (1 - F) * x

    def coupling(self, f, x, absolute=False):
        """Row field f, column field 1 - f."""
        x = np.asarray(x).astype(self.dtype)
        y = self.free[f] * self._ba(0.0, self.b, self.free[1 - f] * x, absolute)
        return y if absolute else -y

    def apply(self, which: str, x, absolute=False):
        n = self.n
        if which == "A11":
            return self.diag_block(0, x, absolute)
        if which == "A22":
            return self.diag_block(1, x, absolute)
        if which == "A12":
            return self.coupling(0, x, absolute)
        if which == "A21":
            return self.coupling(1, x, absolute)
        assert which == "MONO"
        return np.concatenate([self.diag_block(0, x[:n], absolute) + self.coupling(0, x[n:], absolute),
                               self.diag_block(1, x[n:], absolute) + self.coupling(1, x[:n], absolute)])

    def u0(self):
        return np.concatenate([np.where(m, gg, 0.0) for m, gg in zip(self.masks, self.g)])

    def rhs(self, absolute=False):
        """-F A_shifted,unel u0 (absolute: its row-wise magnitude)."""
        r = self.unel(self.u0(), absolute)
        r = np.concatenate(self.free) * r
        return r if absolute else -r

    def step_rhs(self, p, absolute=False):
        """b = -F A_unel p, the UNSHIFTED operator."""
        r = np.concatenate(self.free) * self.unel(np.asarray(p), absolute, sigma=(0.0, 0.0))
        return r if absolute else -r

    def diag(self, f, absolute=False):
        d = diagonal(self.kind, self.nd, self.cK[f], self.cM[f], absolute)
        return np.where(self.masks[f], 1.0, d)


def worst_fraction(got, ref, bound) -> float:
    """max_i |got_i - ref_i| / bound_i (rows of bound 0 must agree exactly: inf otherwise)."""
    d = abs(np.asarray(got) - np.asarray(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(q.max())


# ---------------------------------------------------------------------------------------------------------------------
# launch rules (perphil_amd/csrc/pph_assemble.hip: pph_launch_fused_kernels; pph_transient.hip), restated
# ---------------------------------------------------------------------------------------------------------------------
BLOCK = 256
ASM_TILE_MIN_NODES = 30000       # option asm_tile_min_nodes: levels below it take the two-pass kernels
ASM_NODE_SPLIT_MIN = 200000      # option asm_node_split_min: node kernel in two launches from here on
NODE_MAX_NODES = 1 << 29
TILE_MAX_WG = 4096               # k_asm_tile
TWO_PASS_MAX_WG = 4096           # k_elem_rows, k_gather_rows
SIMPLEX_MAX_WG = 8192            # k_asm_simplex_gather
NODE_MAX_WG = 16384              # k_asm_node2
STEP_MAX_WG = 2048               # k_step_rhs, k_step_constrain, k_step_update (and the live slots of k_step_sum)
TILE = {2: (16, 8, 1), 3: (8, 4, 2)}


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def assembly_path(kind: int, n: int, one_mass: bool, asm_node: int = 1, asm_tile: int = 1, ell: bool = True) -> str:
    """'simplex' | 'node' | 'tile' | 'two-pass' for a level of n nodes.  one_mass: both fields carry the same mass
    coefficient (sigma1 == sigma2 == 0).  The node kernel serves one mass coefficient and stencil-ELL output only."""
    if kind in (TRI, TET):
        return "simplex"
    if one_mass and asm_node and asm_tile and ell and n < NODE_MAX_NODES:
        return "node"
    if asm_tile and (asm_tile == 2 or n >= ASM_TILE_MIN_NODES):
        return "tile"
    return "two-pass"


def tile_counts(kind: int, nd: Sequence[int]) -> Tuple[int, int, int]:
    t = TILE[dim_of(kind)]
    p = [q + 1 for q in nd] + [1] * (3 - len(nd))
    return tuple(_cdiv(p[e], t[e]) for e in range(3))


def tile_launch(kind: int, nd: Sequence[int], xmap: int = 0) -> Dict[str, int]:
    """k_asm_tile: grid = min(ntiles, 4096); option asm_tile_xmap (taken from 64 workgroups on): grid &= ~7, every XCD
    (workgroup % 8) owns tpx = ceil(ntiles / 8) consecutive tiles and its grid / 8 workgroups stride through them."""
    tc = tile_counts(kind, nd)
    ntiles = tc[0] * tc[1] * tc[2]
    grid = min(ntiles, TILE_MAX_WG)
    xm = 1 if (xmap and grid >= 64) else 0
    if xm:
        grid &= ~7
        tpx, step = _cdiv(ntiles, 8), grid >> 3
        passes = _cdiv(tpx, step)
    else:
        tpx, step = ntiles, grid
        passes = _cdiv(ntiles, grid)
    return {"ntiles": ntiles, "grid": grid, "xmap": xm, "tpx": tpx, "step": step, "passes": passes}


def tile_of_nodes(kind: int, nd: Sequence[int]) -> np.ndarray:
    t = TILE[dim_of(kind)]
    tc = tile_counts(kind, nd)
    i, j, k = node_ijk(nd)
    return (i // t[0]) + tc[0] * ((j // t[1]) + tc[1] * (k // t[2]))


def tile_pass(tile: np.ndarray, L: Dict[str, int]) -> np.ndarray:
    """The pass of its workgroup's loop in which a tile is assembled."""
    return (tile % L["tpx"]) // L["step"] if L["xmap"] else tile // L["step"]


def two_pass_launch(kind: int, nd: Sequence[int]) -> Dict[str, int]:
    """k_elem_rows (cells) and k_gather_rows (nodes): batches of 256 / 2^dim, at most 4096 workgroups each."""
    per = BLOCK >> dim_of(kind)
    n, ncell = num_nodes(nd), int(np.prod(nd))
    nbn, nbc = _cdiv(n, per), _cdiv(ncell, per)
    gn, gc = min(nbn, TWO_PASS_MAX_WG), min(nbc, TWO_PASS_MAX_WG)
    return {"per": per, "node_batches": nbn, "cell_batches": nbc, "node_grid": gn, "cell_grid": gc,
            "node_passes": _cdiv(nbn, gn), "cell_passes": _cdiv(nbc, gc)}


def thread_launch(items: int, max_wg: int) -> Dict[str, int]:
    """One work item per thread, grid-stride: grid = min(ceil(items / 256), max_wg)."""
    grid = max(1, min(_cdiv(items, BLOCK), max_wg))
    return {"grid": grid, "stride": grid * BLOCK, "passes": _cdiv(items, grid * BLOCK)}


def simplex_launch(n: int) -> Dict[str, int]:
    return thread_launch(n, SIMPLEX_MAX_WG)


def step_rhs_launch(n: int) -> Dict[str, int]:
    return thread_launch(n, STEP_MAX_WG)


def step_update_launch(n: int) -> Dict[str, int]:
    """k_step_constrain and k_step_update run over the 2n entries of the mixed field; k_step_sum adds `grid` partial sums."""
    return thread_launch(2 * n, STEP_MAX_WG)


def node_launch(n: int) -> Dict[str, int]:
    """k_asm_node2 in one launch: ceil(n / 256) workgroups rounded up to a multiple of 8, at most 16 384; from
    asm_node_split_min nodes on two launches over windows of 64 rows, 4 per workgroup, each capped alike."""
    nb = _cdiv(_cdiv(n, BLOCK), 8) * 8
    grid = min(nb, NODE_MAX_WG)
    return {"grid": grid, "stride": grid * BLOCK, "passes": _cdiv(n, grid * BLOCK), "split": int(n >= ASM_NODE_SPLIT_MIN),
            "windows_per_launch": NODE_MAX_WG * 4}


def mono_launch(n: int) -> Dict[str, int]:
    """blocks_mono: k_mono_rowptr over n + 1 entries on at most 4096 x 256 threads; k_mono_fill with 8 lanes per row (32 rows
    per workgroup) on at most 4096 workgroups."""
    g2 = min(_cdiv(n + 1, BLOCK), 4096)
    gf = min(_cdiv(n * 8, BLOCK), 4096)
    return {"rowptr_grid": g2, "rowptr_passes": _cdiv(n + 1, g2 * BLOCK), "fill_grid": gf, "fill_passes": _cdiv(n, gf * (BLOCK // 8))}


def last_pass_rows(kind: int, nd: Sequence[int], path: str, xmap: int = 0) -> np.ndarray:
    """Boolean per node: assembled in the LAST pass of its kernel's loop (tile loop, node batches, node per thread)."""
    n = num_nodes(nd)
    idx = np.arange(n)
    if path == "tile":
        L = tile_launch(kind, nd, xmap)
        return tile_pass(tile_of_nodes(kind, nd), L) == L["passes"] - 1
    if path == "two-pass":
        L = two_pass_launch(kind, nd)
        return (idx // L["per"]) // L["node_grid"] == L["node_passes"] - 1
    L = {"simplex": simplex_launch, "node": node_launch, "step": step_rhs_launch}[path](n)
    return idx // L["stride"] == L["passes"] - 1


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the GPU file: meshes, Dirichlet sets, data
# ---------------------------------------------------------------------------------------------------------------------
# cell counts are powers of two: the device integrates on stored coordinates i / n, exact only then
# (tests/test_transient_gpu.py::test_more_nodes_than_one_pass_of_the_grid); the node counts are odd, so the last tile is
# partly filled in every direction
SHIFTED = {"hex128x64x64": (HEX, (128, 64, 64)), "quad1024x512": (QUAD, (1024, 512)),
           "tri2048x1024": (TRI, (2048, 1024)), "tet128": (TET, (128, 128, 128))}
UNSHIFTED_ONLY = {"quad2048": (QUAD, (2048, 2048)), "hex256x128x128": (HEX, (256, 128, 128))}
CASES = {**SHIFTED, **UNSHIFTED_ONLY}
INTERIOR_PICKS = 24


def dirichlet_sets(kind: int, nd: Sequence[int], seed: int = 41):
    """Field 0: the whole boundary.  Field 1: the sides x = 0 and y = 1 plus INTERIOR_PICKS seeded interior nodes and the last
    interior node (nx - 1, ny - 1[, nz - 1])."""
    i, j, k = node_ijk(nd)
    dim = len(nd)
    bnd = (i == 0) | (i == nd[0]) | (j == 0) | (j == nd[1])
    if dim == 3:
        bnd |= (k == 0) | (k == nd[2])
    inner = np.nonzero(~bnd)[0]
    m1 = (i == 0) | (j == nd[1])
    if inner.size:
        m1[np.random.default_rng(seed).choice(inner, min(INTERIOR_PICKS, max(1, inner.size // 3)), replace=False)] = True
        m1[inner[-1]] = True
    return np.nonzero(bnd)[0], np.nonzero(m1)[0]


def dirichlet_data(n: int, nodes, seed: int = 43):
    """Values uniform in [0.5, 1.5] on the constrained nodes, 0 elsewhere."""
    rng = np.random.default_rng(seed)
    g = (np.zeros(n), np.zeros(n))
    for f in (0, 1):
        g[f][nodes[f]] = rng.uniform(0.5, 1.5, len(nodes[f]))
    return g


def dominant_sigma(cf, nx: int) -> Tuple[float, float]:
    """tests/test_transient_gpu.py::_dominant_sigma: sigma h^2 about 10 k on the fine level, different for the two fields."""
    return 10.0 * cf.k1 / cf.mu * nx * nx, 10.0 * cf.k2 / cf.mu * nx * nx


def probe_vectors(n: int, last: np.ndarray, seed: int):
    """Two seeded normal vectors and one that is nonzero on the rows of the last pass only."""
    rng = np.random.default_rng(seed)
    v = [rng.standard_normal(n), rng.standard_normal(n)]
    z = rng.standard_normal(n)
    z[~last] = 0.0
    return v + [z]


def within_bar(got, ref, bound) -> bool:
    """The row-wise comparison of the GPU file: |got_i - ref_i| <= BAR bound_i."""
    return worst_fraction(got, ref, BAR * np.asarray(bound)) <= 1.0


def norm_check(got: float, vec: np.ndarray) -> Tuple[float, float]:
    """(relative difference of got^2 from the fp64 sum of squares of vec, its bound max(100 delta, 1e-13)): the rule of the
    error norms (tests/README.md), on the squared sums."""
    want = float(np.dot(vec, vec))
    return abs(got * got - want) / want, max(100.0 * sum_drift(vec), 1e-13)


def sum_drift(v: np.ndarray) -> float:
    """delta: relative difference of the fp64 sum of squares against its longdouble self."""
    s64 = float(np.dot(v, v))
    sl = np.dot(v.astype(np.longdouble), v.astype(np.longdouble))
    return float(abs(np.longdouble(s64) - sl) / sl) if sl > 0 else 0.0


def residual_drift(kind: int, theta: float, seed: int = 3) -> float:
    """The reference's own error in evaluating a step's residual r = (Sigma M / dt + theta A) d - b: fp64 against longdouble,
    ||D^-1 (r64 - rld)|| / ||D^-1 b||, on the small ragged mesh of the kind with d the direct solution (so that, as in a
    converged step, the two terms of r cancel) and the dominant shift of the GPU cases."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    nd = dict((k, d) for k, d in SMALL[:4])[kind]
    n = num_nodes(nd)
    nodes = dirichlet_sets(kind, nd)
    masks = T.masks_of(n, *nodes)
    g = dirichlet_data(n, nodes)
    sig = dominant_sigma(CF, nd[0])
    step_cf = T.Coefs(theta * CF.k1, theta * CF.k2, theta * CF.beta, CF.mu)
    p = np.random.default_rng(seed).standard_normal(2 * n)
    K, M = T.matfree_scalar_matrices(kind, *nd)
    A11, A22, A12, A21, _, _ = T.shifted_blocks(K, M, step_cf, sig, masks, g)
    b = System(kind, nd, CF, (0.0, 0.0), masks, g).step_rhs(p)
    d = spla.spsolve(sp.bmat([[A11, A12], [A21, A22]], format="csc"), b)
    d[np.concatenate(masks)] = 0.0
    out = []
    for dtype in (np.float64, np.longdouble):
        S = System(kind, nd, step_cf, sig, masks, g, dtype)
        out.append(S.apply("MONO", d.astype(dtype)) - System(kind, nd, CF, (0.0, 0.0), masks, g, dtype).step_rhs(p.astype(dtype)))
    S = System(kind, nd, step_cf, sig, masks, g)
    dinv = 1.0 / np.concatenate([S.diag(0), S.diag(1)])
    return float(np.linalg.norm(dinv * (out[0] - out[1]).astype(np.float64)) / np.linalg.norm(dinv * b))
