"""Vectorised, matrix-free restatement of the degree-2 (Q2 / P2) discretisation for meshes too large for the cell loops of
tests/p2_restatement.py (test infrastructure only).  Written from the documented conventions (pph_p2.h, p2_restatement's
module docstring), not from the library's code:

* dofmap_fast: the cell->dof map by broadcasting over boxes x sub-cells x local lattice offsets;
* row_lengths: the row lengths of the scalar CSR pattern by a closed form (the length factors into per-direction node
  classes: first point, last point, odd point, even interior point), and the pattern itself for moderate meshes;
* element_matrices_by_subcell: the meshes are uniform, so one K_e / M_e pair per sub-cell type (1 / 2 / 1 / 6);
* apply_KM / apply_blocks / lift: y = (cK K + cM M) x, the Dirichlet-eliminated DPP blocks and the lifted right-hand side
  by gather, einsum and np.bincount, each with the row-wise magnitude sum (|cK K_e| + |cM M_e|) |x| that the
  rounding-error bounds of the GPU tests are built from;
* norms_reference: the squared L2 / H1-seminorm errors with the Gauss rule of k_error_norms_p2 (nq points per direction,
  collapsed onto the simplex), in chunks of cells, with the magnitude sums the tolerance needs;
* ilu0 / ilu_apply in any NumPy float type, for the longdouble discrepancy of the ILU(0) restatement.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import p2_restatement as R  # noqa: E402

U = 2.0 ** -53           # unit roundoff of fp64


def dims3(kind, nx, ny, nz=0):
    return nx, ny, (nz if R.dim_of(kind) == 3 else 1)


def local_lattice_ids(kind, nx, ny, nz=0):
    """[cells_per_box, m] offsets of the local nodes of each sub-cell from the box's lowest lattice point (node ids)."""
    px, py, _ = R.lattice_dims(kind, nx, ny, nz)
    return np.array([[o[0] + px * (o[1] + py * o[2]) for o in R.local_offsets(kind, s)]
                     for s in range(R.cells_per_box(kind))], dtype=np.int64)


def box_base(kind, nx, ny, nz=0, b0=0, b1=None):
    """Lattice id of the lowest point of boxes [b0, b1) (box id = bx + nx (by + ny bz))."""
    px, py, _ = R.lattice_dims(kind, nx, ny, nz)
    nbox = nx * ny * dims3(kind, nx, ny, nz)[2]
    b = np.arange(b0, nbox if b1 is None else b1, dtype=np.int64)
    bx, t = b % nx, b // nx
    by, bz = t % ny, t // ny
    return 2 * bx + px * (2 * by + py * 2 * bz)


def dofmap_fast(kind, nx, ny, nz=0):
    cells = box_base(kind, nx, ny, nz)[:, None, None] + local_lattice_ids(kind, nx, ny, nz)[None]
    return cells.reshape(-1, R.nodes_per_cell(kind)).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------------------
# pattern
# ----------------------------------------------------------------------------------------------------------------------
def _node_class(I, P):
    """0: first point, 1: last point, 2: odd point (inside one box along this direction), 3: even interior point."""
    c = np.where(I % 2 == 1, 2, 3)
    c = np.where(I == P - 1, 1, c)
    return np.where(I == 0, 0, c)


_CLASS_TABLES = {}


def _class_table(kind):
    """Row length per tuple of direction classes, read off the loop pattern of a 2 x 2 (x 2) mesh, where every class tuple
    occurs (the row of a node sees only the boxes within one lattice step of it: the length depends on its classes only)."""
    if kind not in _CLASS_TABLES:
        d = R.dim_of(kind)
        nx, ny, nz = 2, 2, (2 if d == 3 else 0)
        rowptr, _ = R.pattern(kind, nx, ny, nz)
        lens = np.diff(rowptr)
        px, py, pz = R.lattice_dims(kind, nx, ny, nz)
        ids = np.arange(px * py * pz)
        cls = [_node_class(ids % px, px), _node_class((ids // px) % py, py)] + ([_node_class(ids // (px * py), pz)] if d == 3 else [])
        tab = np.full((4,) * d, -1, dtype=np.int64)
        for i in range(ids.size):
            key = tuple(int(c[i]) for c in cls)
            assert tab[key] in (-1, lens[i])
            tab[key] = lens[i]
        assert (tab > 0).all()
        _CLASS_TABLES[kind] = tab
    return _CLASS_TABLES[kind]


def row_lengths(kind, nx, ny, nz=0):
    """Row lengths of the scalar pattern (int64 [n]); Q2: the product of the per-direction counts 3 / 3 / 3 / 5."""
    px, py, pz = R.lattice_dims(kind, nx, ny, nz)
    tab = _class_table(kind)
    cx = _node_class(np.arange(px), px)
    cy = _node_class(np.arange(py), py)
    if R.dim_of(kind) == 2:
        return tab[cx[None, :], cy[:, None]].reshape(-1)
    cz = _node_class(np.arange(pz), pz)
    return tab[cx[None, None, :], cy[None, :, None], cz[:, None, None]].reshape(-1)


def nnz_closed_form(kind, nx, ny, nz=0):
    """Entries of the scalar block; Q2 hex N1 x N2 x N3: (8 N1 + 1)(8 N2 + 1)(8 N3 + 1), Q2 quad (8 N1 + 1)(8 N2 + 1)
    (per direction: N - 1 even interior points of 5, two ends of 3, N odd points of 3)."""
    if kind in (R.QUAD, R.HEX):
        out = 1
        for N in ([nx, ny] if kind == R.QUAD else [nx, ny, nz]):
            out *= 8 * N + 1
        return out
    return int(row_lengths(kind, nx, ny, nz).sum())


def max_row(kind):
    return int(_class_table(kind).max())


def pattern_fast(kind, nx, ny, nz=0, chunk=1 << 18):
    """Sorted CSR pattern (rowptr int64, col int32) from the cell pairs, in chunks of boxes."""
    n = R.n_nodes(kind, nx, ny, nz)
    loc = local_lattice_ids(kind, nx, ny, nz)
    nbox = nx * ny * dims3(kind, nx, ny, nz)[2]
    P = sp.csr_matrix((n, n), dtype=np.int8)
    for b0 in range(0, nbox, chunk):
        c = (box_base(kind, nx, ny, nz, b0, min(b0 + chunk, nbox))[:, None, None] + loc[None]).reshape(-1, loc.shape[1])
        r = np.repeat(c, c.shape[1], axis=1).ravel()
        cc = np.tile(c, (1, c.shape[1])).ravel()
        Q = sp.csr_matrix((np.ones(r.size, dtype=np.int8), (r, cc)), shape=(n, n))
        Q.data[:] = 1
        P = P + Q
        P.data[:] = 1
    P.sort_indices()
    return P.indptr.astype(np.int64), P.indices.astype(np.int32)


# ----------------------------------------------------------------------------------------------------------------------
# element matrices and products
# ----------------------------------------------------------------------------------------------------------------------
def element_matrices_by_subcell(kind, nx, ny, nz=0):
    """[(K_e, M_e)] per sub-cell type of the uniform mesh (frame vertices at their lattice offsets / (2 n))."""
    scale = np.array([2.0 * nx, 2.0 * ny, 2.0 * max(nz, 1)])
    d = R.dim_of(kind)
    out = []
    for s in range(R.cells_per_box(kind)):
        offs = np.array(R.local_offsets(kind, s), dtype=float)
        F = offs[R.frame_locals(kind)][:, :d] / scale[:d]
        out.append(R.element_matrices(kind, F))
    return out


class Operator:
    """The mesh's element matrices and cell->dof map, for repeated matrix-free products."""

    def __init__(self, kind, nx, ny, nz=0, elems=None):
        self.kind, self.dims = kind, (nx, ny, nz)
        self.n = R.n_nodes(kind, nx, ny, nz)
        self.cpb, self.m = R.cells_per_box(kind), R.nodes_per_cell(kind)
        self.cells = dofmap_fast(kind, nx, ny, nz).reshape(-1, self.cpb, self.m)
        self.elems = elems if elems is not None else element_matrices_by_subcell(kind, nx, ny, nz)

    def parts(self, x, dtype=np.float64):
        """K x, M x, |K| |x|, |M| |x| (sums of the element contributions in box order)."""
        out = [np.zeros(self.n, dtype=dtype) for _ in range(4)]
        ax = np.abs(x)
        for s, (Ke, Me) in enumerate(self.elems):
            c = self.cells[:, s, :]
            flat = c.ravel()
            xe, axe = x[c], ax[c]
            for k, (A, v) in enumerate([(Ke, xe), (Me, xe), (np.abs(Ke), axe), (np.abs(Me), axe)]):
                out[k] += np.bincount(flat, weights=(v @ A.T.astype(dtype)).ravel(), minlength=self.n)
        return out


def apply_KM(kind, dims, x, cK, cM, op=None):
    """y = (cK K + cM M) x and mag = (|cK K_e| + |cM M_e|) |x| summed over the cells."""
    op = op or Operator(kind, *dims)
    Kx, Mx, aK, aM = op.parts(np.asarray(x, dtype=float))
    return cK * Kx + cM * Mx, abs(cK) * aK + abs(cM) * aM


def block_coefs(k1, k2, beta, mu):
    """(cK, cM) of A11, A22, A12 = A21 before elimination."""
    return {"A11": (k1 / mu, beta / mu), "A22": (k2 / mu, beta / mu), "A12": (0.0, -beta / mu), "A21": (0.0, -beta / mu)}


def apply_blocks(kind, dims, mask, x1, x2, k1, k2, beta, mu, op=None):
    """Products of the eliminated blocks F A F + I_b (A12, A21: F A F) and of the monolithic matrix, with magnitudes:
    {"K": K x1, "M": M x1, "A11": A11 x1, "A22": A22 x2, "A12": A12 x2, "A21": A21 x1, "MONO": MONO [x1; x2]}, each
    (y, mag)."""
    op = op or Operator(kind, *dims)
    keep = (~np.asarray(mask, bool)).astype(float)
    bnd = 1.0 - keep
    K1, M1, aK1, aM1 = op.parts(x1)
    P1 = op.parts(keep * x1)
    P2 = op.parts(keep * x2)
    cf = block_coefs(k1, k2, beta, mu)

    def blk(name, P, x, ident):
        (cK, cM), (Kx, Mx, aK, aM) = cf[name], P
        y = keep * (cK * Kx + cM * Mx)
        mag = keep * (abs(cK) * aK + abs(cM) * aM)
        if ident:
            y, mag = y + bnd * x, mag + bnd * np.abs(x)
        return y, mag

    out = {"K": (K1, aK1), "M": (M1, aM1), "A11": blk("A11", P1, x1, True), "A22": blk("A22", P2, x2, True),
           "A12": blk("A12", P2, x2, False), "A21": blk("A21", P1, x1, False)}
    a11, a12 = out["A11"], out["A12"]
    a21, a22 = out["A21"], out["A22"]
    out["MONO"] = (np.concatenate([a11[0] + a12[0], a21[0] + a22[0]]), np.concatenate([a11[1] + a12[1], a21[1] + a22[1]]))
    return out


def lift(kind, dims, mask, G1, G2, k1, k2, beta, mu, op=None):
    """Lifted right-hand side r = -F (A G) of R.eliminate (0 on constrained rows) with its magnitude, and u0 = G."""
    op = op or Operator(kind, *dims)
    keep = (~np.asarray(mask, bool)).astype(float)
    P1, P2 = op.parts(G1), op.parts(G2)
    cf = block_coefs(k1, k2, beta, mu)

    def prod(name, P):
        (cK, cM), (Kx, Mx, aK, aM) = cf[name], P
        return cK * Kx + cM * Mx, abs(cK) * aK + abs(cM) * aM

    (y11, m11), (y12, m12), (y21, m21), (y22, m22) = prod("A11", P1), prod("A12", P2), prod("A21", P1), prod("A22", P2)
    r = np.concatenate([-keep * (y11 + y12), -keep * (y21 + y22)])
    mag = np.concatenate([keep * (m11 + m12), keep * (m21 + m22)])
    return r, mag, np.concatenate([G1, G2])


def spmv_bound_factor(max_row_len, dim):
    """c of |y - y_ref|_i <= c u mag_i: at most 8 incident boxes add entries of at most D^2 + 2 table terms, the CSR sum runs
    over at most max_row terms, times a margin of 4."""
    return 4.0 * (max_row_len + 8 * (dim * dim + 2))


def row_excess(y, y_ref, mag, c):
    """max_i |y - y_ref|_i / (c u mag_i) (the check passes when <= 1; a row with mag 0 must match exactly)."""
    diff = np.abs(np.asarray(y) - np.asarray(y_ref))
    lim = c * U * np.asarray(mag)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(lim > 0, diff / np.where(lim > 0, lim, 1.0), np.where(diff > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


def rel_max_error(z, ref):
    """max |z - ref| / max |ref| (the p-multigrid cycle comparisons)."""
    return float(np.max(np.abs(np.asarray(z) - np.asarray(ref))) / np.max(np.abs(ref)))


# ----------------------------------------------------------------------------------------------------------------------
# error norms
# ----------------------------------------------------------------------------------------------------------------------
def norm_rule(kind, nq):
    """Reference points [npts, d] and weights of k_error_norms_p2: Gauss on [-1, 1] mapped to [0, 1] (weight / 2 per
    direction), collapsed onto the simplex for triangles / tetrahedra; point q = (q % nq, q / nq % nq, q / nq^2)."""
    x, w = np.polynomial.legendre.leggauss(nq)
    d = R.dim_of(kind)
    pts, wts = [], []
    for q in range(nq ** d):
        qi = [q % nq, (q // nq) % nq, q // (nq * nq)][:d]
        if kind in (R.QUAD, R.HEX):
            pts.append([0.5 * (x[i] + 1.0) for i in qi])
            wts.append(np.prod([0.5 * w[i] for i in qi]))
            continue
        u, v = 0.5 * (x[qi[0]] + 1.0), 0.5 * (x[qi[1]] + 1.0)
        wt = 0.25 * w[qi[0]] * w[qi[1]] * (1.0 - u)
        p = [u, v * (1.0 - u)]
        if d == 3:
            t = 0.5 * (x[qi[2]] + 1.0)
            p.append(t * (1.0 - u) * (1.0 - v))
            wt *= 0.5 * w[qi[2]] * (1.0 - u) * (1.0 - v)
        pts.append(p)
        wts.append(wt)
    return np.array(pts), np.array(wts)


def norms_reference(kind, dims, nodal, exact, grad, nq, chunk=1 << 15, cell_range=None, rule=None, want_points=False):
    """Squared L2 and H1-seminorm errors of the degree-2 nodal field against exact / grad over the cells (all, or
    [c0, c1)), with the magnitude sums of the tolerance: dict l2, h1, S_l2 = sum_q wd |du| A_q, S_h1 = sum_q wd sum_d
    |dg_d| A_qd, where A_q = sum_b |N_b U_b| + |p| and A_qd = sum_e |J^-1|_ed sum_b |dN_be U_b| + |g_d|; wd = w |det J|."""
    nx, ny, nz = dims
    d = R.dim_of(kind)
    pts, wts = rule if rule is not None else norm_rule(kind, nq)
    basis = [R.basis(kind, p) for p in pts]
    Nq = np.array([b[0] for b in basis])             # [npts, m]
    Gq = np.array([b[1] for b in basis])             # [npts, m, d]
    cells = dofmap_fast(kind, nx, ny, nz)
    c0, c1 = cell_range if cell_range is not None else (0, cells.shape[0])
    px, py, _ = R.lattice_dims(kind, nx, ny, nz)
    scale = np.array([2.0 * nx, 2.0 * ny, 2.0 * max(nz, 1)])[:d]
    frame = R.frame_locals(kind)
    nodal = np.asarray(nodal, dtype=float)
    acc = dict(l2=0.0, h1=0.0, S_l2=0.0, S_h1=0.0)
    xs = []
    for a in range(c0, c1, chunk):
        c = cells[a:min(a + chunk, c1)].astype(np.int64)
        ids = c[:, frame]
        Xf = np.stack([ids % px, (ids // px) % py] + ([ids // (px * py)] if d == 3 else []), axis=-1) / scale   # [C, d+1, d]
        J = np.transpose(Xf[:, 1:, :] - Xf[:, :1, :], (0, 2, 1))      # J[c, dd, e] = X_{e+1}[dd] - X_0[dd]
        det = np.abs(np.linalg.det(J))
        Ji = np.linalg.inv(J)                                           # Ji[c, e, dd]
        Uc = nodal[c]                                                   # [C, m]
        uh = Uc @ Nq.T                                                  # [C, npts]
        gr = np.einsum("cm,qme->cqe", Uc, Gq)                           # reference gradient
        gh = np.einsum("ced,cqe->cqd", Ji, gr)                          # J^-T grad_ref
        xq = Xf[:, 0, None, :] + np.einsum("cde,qe->cqd", J, pts)
        flat = xq.reshape(-1, d)
        pe = np.asarray(exact(flat), dtype=float).reshape(uh.shape)
        ge = np.asarray(grad(flat), dtype=float).reshape(gh.shape)
        wd = wts[None, :] * det[:, None]
        du, dg = uh - pe, gh - ge
        A = np.abs(Uc[:, None, :] * Nq[None]).sum(-1) + np.abs(pe)
        Ag = np.einsum("ced,cqe->cqd", np.abs(Ji), np.abs(Uc[:, None, :, None] * Gq[None]).sum(2)) + np.abs(ge)
        acc["l2"] += float(np.sum(wd * du * du))
        acc["h1"] += float(np.sum(wd[..., None] * dg * dg))
        acc["S_l2"] += float(np.sum(wd * np.abs(du) * A))
        acc["S_h1"] += float(np.sum(wd[..., None] * np.abs(dg) * Ag))
        if want_points:
            xs.append(flat)
    if want_points:
        acc["points"] = np.concatenate(xs) if xs else np.zeros((0, d))
    return acc


def norms_bound(ref, kind, ncell, nq, count=None):
    """Allowed |Delta| on the squared L2 / H1 norms: u (2 (NB + 20) S + L sq), L = ceil(count / (grid 256)) npts + 2304
    (grid = min(ceil(count / 256), 2048) workgroups of 256 lanes: the per-lane chain, then the block and final sums)."""
    count = ncell if count is None else count
    npts = nq ** R.dim_of(kind)
    grid = min(-(-count // 256), 2048)
    L = -(-count // (grid * 256)) * npts + 2304
    NB = R.nodes_per_cell(kind)
    return (U * (2 * (NB + 20) * ref["S_l2"] + L * ref["l2"]), U * (2 * (NB + 20) * ref["S_h1"] + L * ref["h1"]), L)


def norms_excess(got_sq, ref, bound):
    """max over the two squared norms of |got - ref| / bound (the check passes when <= 1)."""
    return max(abs(got_sq[0] - ref["l2"]) / bound[0], abs(got_sq[1] - ref["h1"]) / bound[1])


def mms_exact(field, dim, k1, k2, beta, mu):
    """The manufactured pressure `field` (0 / 1) and its gradient, as callables of point arrays."""
    eta = math.sqrt(beta * (k1 + k2) / (k1 * k2))
    ce = -mu / (beta * k1) if field == 0 else mu / (beta * k2)

    def p(X):
        ex = np.exp(math.pi * X[:, 0])
        if dim == 2:
            return (mu / math.pi) * ex * np.sin(math.pi * X[:, 1]) + ce * np.exp(eta * X[:, 1])
        return ((mu / math.pi) * ex * (np.sin(math.pi * X[:, 1]) + np.sin(math.pi * X[:, 2]))
                + ce * (np.exp(eta * X[:, 1]) + np.exp(eta * X[:, 2])))

    def g(X):
        ex = np.exp(math.pi * X[:, 0])
        if dim == 2:
            return np.stack([mu * ex * np.sin(math.pi * X[:, 1]),
                             mu * ex * np.cos(math.pi * X[:, 1]) + ce * eta * np.exp(eta * X[:, 1])], axis=1)
        return np.stack([mu * ex * (np.sin(math.pi * X[:, 1]) + np.sin(math.pi * X[:, 2])),
                         mu * ex * np.cos(math.pi * X[:, 1]) + ce * eta * np.exp(eta * X[:, 1]),
                         mu * ex * np.cos(math.pi * X[:, 2]) + ce * eta * np.exp(eta * X[:, 2])], axis=1)

    return p, g


# ----------------------------------------------------------------------------------------------------------------------
# ILU(0) in any float type
# ----------------------------------------------------------------------------------------------------------------------
def ilu0(A, dtype=np.float64):
    """IKJ ILU(0) on the pattern of A (explicit zeros kept), natural order, arithmetic in `dtype` (R.ilu0 restated)."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    ip, ix = A.indptr, A.indices
    LU = A.data.astype(dtype)
    diag = np.array([ip[i] + np.searchsorted(ix[ip[i]:ip[i + 1]], i) for i in range(n)])
    for i in range(n):
        row = {int(ix[k]): k for k in range(ip[i], ip[i + 1])}
        for k in range(ip[i], diag[i]):
            j = int(ix[k])
            LU[k] /= LU[diag[j]]
            for kk in range(diag[j] + 1, ip[j + 1]):
                t = row.get(int(ix[kk]))
                if t is not None:
                    LU[t] -= LU[k] * LU[kk]
    return ip, ix, LU, diag


def ilu_apply(fac, r):
    ip, ix, LU, diag = fac
    y = np.array(r, dtype=LU.dtype)
    for i in range(len(y)):
        y[i] -= np.sum(LU[ip[i]:diag[i]] * y[ix[ip[i]:diag[i]]])
    for i in range(len(y) - 1, -1, -1):
        s, e = diag[i] + 1, ip[i + 1]
        y[i] = (y[i] - np.sum(LU[s:e] * y[ix[s:e]])) / LU[diag[i]]
    return y
