"""Plain fp64 NumPy restatement of what pph_post.hip computes for CG-1 fields: the squared L2 / H1-seminorm error sums
(k_error_norms, k_error_norms_simplex) and the Darcy projection (k_darcy_rhs_*, the mass-matrix solve).  Vectorised,
walking the cells in blocks of bounded memory, so that meshes past the kernels' launch caps (12 M tetrahedra) are
feasible.  Everything takes the cell->node map and the coordinates as arrays: a test passes the device's own.  Nothing
here imports the product package or the oracle.

Error sums: tensor Gauss rule with nq points per direction (np.polynomial.legendre.leggauss), point q = q0 + nq q1 +
nq^2 q2 with q_e the index along reference direction e; on simplices collapsed by the Duffy map lambda_1 = u,
lambda_2 = v (1 - u), lambda_3 = w (1 - u)(1 - v), as oracle.dpp_oracle.error_norms does.  Every array is of the working
type, np.float64 or np.longdouble (`longdouble=True`), including the exact field: the two runs evaluate the same
function of the same fp64 inputs, and their discrepancy is the rounding of the fp64 evaluation.

Launch rules restated from pph_post.hip (norms_mms, norms_sampled, pph_quadrature_points: grid = min(ceil(cells / 256),
2048); darcy: grid = min(ceil(n / 256), 8192)): norm_launch, darcy_launch."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.linalg as sla

QUAD, TRI, HEX, TET = 0, 1, 2, 3
KIND_NAME = {QUAD: "quad", TRI: "tri", HEX: "hex", TET: "tet"}
U = 2.0 ** -53
WORKERS = min(8, os.cpu_count() or 1)

# pph_post.hip: 256 lanes per workgroup; at most 2048 workgroups in the norm kernels, 8192 in the projection's
BLOCK, NORM_GRID_CAP, DARCY_GRID_CAP = 256, 2048, 8192
NORM_LANES, DARCY_LANES = NORM_GRID_CAP * BLOCK, DARCY_GRID_CAP * BLOCK      # 524 288 cells, 2 097 152 nodes
# pph_post.hip, darcy(): pph_cg_jacobi(..., rtol 1e-13, atol 0, max_it 1000); pph_solve.hip, cg_solve: res = sqrt(z.z) with
# z = dinv .* r, tol = rtol * (res of the zero guess = ||D^-1 b||_2), stop at res <= tol
CG_RTOL = 1e-13
FLOOR = 1e-13
# smallest eigenvalue of D^-1 M from the element matrices (Wathen 1987: the spectrum of D^-1 M lies between the extreme
# eigenvalues of D_e^-1 M_e): P1 simplices [1/2, 1 + d/2], Q1 quadrilaterals [1/4, 9/4], Q1 hexahedra [1/8, 27/8]
LAMBDA_MIN = {QUAD: 0.25, TRI: 0.5, HEX: 0.125, TET: 0.5}


def dim_of(kind):
    return 2 if kind in (QUAD, TRI) else 3


def n_cells(kind, nx, ny, nz=0):
    return {QUAD: nx * ny, TRI: 2 * nx * ny, HEX: nx * ny * nz, TET: 6 * nx * ny * nz}[kind]


def n_nodes(kind, nx, ny, nz=0):
    return (nx + 1) * (ny + 1) * ((nz + 1) if dim_of(kind) == 3 else 1)


def norm_launch(count):
    """(workgroups, passes of the longest thread) of a norm / quadrature-point launch over `count` cells."""
    grid = min(-(-count // BLOCK), NORM_GRID_CAP)
    return grid, -(-count // (grid * BLOCK))


def darcy_launch(n):
    grid = min(-(-n // BLOCK), DARCY_GRID_CAP)
    return grid, -(-n // (grid * BLOCK))


def norm_slot(cell_in_launch, count):
    """partial-sum slot (workgroup) that the cell with this index within a launch over `count` cells is added to"""
    grid, _ = norm_launch(count)
    return (cell_in_launch % (grid * BLOCK)) // BLOCK


# ----------------------------------------------------------------------------------------------------------------------
# fields
# ----------------------------------------------------------------------------------------------------------------------
def mms_exact(d, k1, k2, beta, mu):
    """X [m, d] -> (P [2, m], G [2, m, d]): both manufactured pressures and their gradients, in the type of X.  The
    constants are the kernel's fp64 ones (PI, mu / PI, eta = sqrt(beta (k1 + k2) / (k1 k2)), -mu / (beta k1), mu / (beta k2))."""
    eta64 = float(np.sqrt(beta * (k1 + k2) / (k1 * k2)))
    coef64 = (-mu / (beta * k1), mu / (beta * k2))
    mop64 = mu / np.pi

    def f(X):
        T = X.dtype.type
        pi, eta, mop, m = T(np.pi), T(eta64), T(mop64), T(mu)
        ex = np.exp(pi * X[:, 0])
        S, Cs, E = np.sin(pi * X[:, 1]), [np.cos(pi * X[:, 1])], [np.exp(eta * X[:, 1])]
        if d == 3:
            S = S + np.sin(pi * X[:, 2])
            Cs.append(np.cos(pi * X[:, 2]))
            E.append(np.exp(eta * X[:, 2]))
        Es = E[0] if d == 2 else E[0] + E[1]
        P = np.empty((2, X.shape[0]), X.dtype)
        G = np.empty((2, X.shape[0], d), X.dtype)
        for fi in range(2):
            c = T(coef64[fi])
            P[fi] = mop * ex * S + c * Es
            G[fi, :, 0] = m * ex * S
            for e in range(1, d):
                G[fi, :, e] = m * ex * Cs[e - 1] + c * eta * E[e - 1]
        return P, G

    return f


def smooth_factor(X):
    """1 + 0.1 s(x), s smooth with |s| <= 1: the perturbation of the interpolant in the well-conditioned cases"""
    s = np.sin(3.0 * X[:, 0] + 1.0) * np.cos(2.0 * X[:, 1] - 0.5)
    if X.shape[1] == 3:
        s = s * np.cos(1.5 * X[:, 2] + 0.25)
    return 1.0 + 0.1 * s


# ----------------------------------------------------------------------------------------------------------------------
# geometry helpers (any float type: np.linalg has no longdouble)
# ----------------------------------------------------------------------------------------------------------------------
def _det_inv(J):
    """determinant and inverse of [..., d, d] by the adjugate"""
    d = J.shape[-1]
    A = np.empty_like(J)
    if d == 2:
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        A[..., 0, 0], A[..., 0, 1] = J[..., 1, 1], -J[..., 0, 1]
        A[..., 1, 0], A[..., 1, 1] = -J[..., 1, 0], J[..., 0, 0]
    else:
        for i in range(3):
            for j in range(3):
                i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                A[..., j, i] = J[..., i1, j1] * J[..., i2, j2] - J[..., i1, j2] * J[..., i2, j1]   # cofactor (i, j), cyclic
        det = J[..., 0, 0] * A[..., 0, 0] + J[..., 0, 1] * A[..., 1, 0] + J[..., 0, 2] * A[..., 2, 0]
    return det, A / det[..., None, None]


def gauss_rule(nq):
    return np.polynomial.legendre.leggauss(nq)


def _tensor_points(nq, d, rule, T):
    x, w = (np.asarray(a).astype(T) for a in rule)
    q = np.arange(nq ** d)
    qi = [q % nq, (q // nq) % nq, q // (nq * nq)][:d]
    return np.stack([x[i] for i in qi], axis=1), np.prod(np.stack([w[i] for i in qi]), axis=0)


def _multilinear_basis(xi):
    """N [q, b], dN [q, b, e] of the 2^d-node cell on [-1, 1]^d; node b sits at the corner with bits (b >> e) & 1"""
    npts, d = xi.shape
    nb = 1 << d
    T = xi.dtype.type
    N = np.ones((npts, nb), xi.dtype)
    dN = np.ones((npts, nb, d), xi.dtype)
    for b in range(nb):
        for e in range(d):
            s = T(1.0) if (b >> e) & 1 else T(-1.0)
            N[:, b] *= T(0.5) * (1 + s * xi[:, e])
            for f in range(d):
                dN[:, b, f] *= (T(0.5) * s) if f == e else T(0.5) * (1 + s * xi[:, e])
    return N, dN


# sums over the few nodes / directions written out as loops of whole-array operations (fast in either float type)
def _interp(N, X):
    """sum_b N[q, b] X[..., c, b, d] -> [..., c, q, d]"""
    return sum(N[:, b, None] * X[..., b, None, :] for b in range(N.shape[1]))


def _jacobian(dN, X):
    """sum_b dN[q, b, e] X[..., c, b, d] -> [..., c, q, e, d]"""
    return sum(dN[:, b, :, None] * X[..., b, None, None, :] for b in range(dN.shape[1]))


def _matvec(I, g):
    """sum_e I[..., d, e] g[k, ..., e] -> [k, ..., d]"""
    return sum(I[None, ..., e] * g[..., None, e] for e in range(I.shape[-1]))


def _cell_quantities(kind, X, Uc, nq, rule):
    """X [c, nb, d], Uc [K, c, nb] -> xq [c, q, d], uh [K, c, q], gh [K, c, q or 1, d], wd [c, q]"""
    T = X.dtype.type
    d = X.shape[-1]
    xi, w = _tensor_points(nq, d, rule, X.dtype)
    if kind in (QUAD, HEX):
        N, dN = _multilinear_basis(xi)
        npts, nb = N.shape
        dNf = np.ascontiguousarray(dN.transpose(1, 0, 2)).reshape(nb, npts * d)          # [b, (q, e)]
        Xt = np.ascontiguousarray(X.transpose(0, 2, 1))                                   # [c, d, b]
        xq = np.dot(Xt, N.T).transpose(0, 2, 1)                                           # [c, q, d]
        J = np.dot(Xt, dNf).reshape(-1, d, npts, d).transpose(0, 2, 3, 1)                 # [c, q, e, d]
        det, I = _det_inv(J)
        uh = np.dot(Uc, N.T)                                                              # [K, c, q]
        gh = _matvec(I, np.dot(Uc, dNf).reshape(Uc.shape[0], -1, npts, d))
        return xq, uh, gh, w[None, :] * np.abs(det)
    uu = T(0.5) * (xi[:, 0] + 1)
    vv = T(0.5) * (xi[:, 1] + 1)
    lam = [uu, vv * (1 - uu)]
    wq = T(0.25) * w * (1 - uu)                           # w = product of the 1D weights
    if d == 3:
        ww = T(0.5) * (xi[:, 2] + 1)
        lam.append(ww * (1 - uu) * (1 - vv))
        wq = wq * T(0.5) * (1 - uu) * (1 - vv)
    lam = np.stack(lam, axis=1)                           # [q, r]
    E = X[:, 1:, :] - X[:, :1, :]                         # [c, r, d]
    dU = Uc[:, :, 1:] - Uc[:, :, :1]                      # [K, c, r]
    det, I = _det_inv(E)
    gh = _matvec(I, dU)[:, :, None, :]
    xq = X[:, None, 0, :] + _interp(lam, E)
    uh = Uc[:, :, :1] + _interp(lam, dU[..., None])[..., 0]
    return xq, uh, gh, wq[None, :] * np.abs(det)[:, None]


def error_sums(kind, cells, coords, nodal, fields, nq, exact=None, samples=None, cell_range=None, block=8192,
               longdouble=False, rule=None, per_cell=False, want_points=False, order=None):
    """Squared L2 and H1-seminorm errors of the nodal CG-1 fields nodal [K, n] over the cells [c0, c1).

    exact: X [m, d] -> (P [F, m], G [F, m, d]); field k is compared with component fields[k].  Or samples = (se, sg):
    se [(c1 - c0) npts], sg [(c1 - c0) npts, d] or None, in the layout of pph_quadrature_points, for every field.
    Neither: the exact field is zero.  block: cells per pass (memory).  order: a permutation of range(c1 - c0) - the cells
    are visited, and their contributions summed, in that order.  rule: (points, weights) instead of leggauss(nq).
    Returns {"l2": [K], "h1": [K]} in the working type, plus "cell_l2" / "cell_h1" [K, c1 - c0] (per_cell) and
    "points" [(c1 - c0) npts, d] (want_points)."""
    T = np.longdouble if longdouble else np.float64
    d = dim_of(kind)
    nodal = np.atleast_2d(np.asarray(nodal, dtype=np.float64))
    K = nodal.shape[0]
    fields = np.asarray(fields, dtype=np.int64)
    c0, c1 = cell_range if cell_range is not None else (0, cells.shape[0])
    count = c1 - c0
    npts = nq ** d
    rule = gauss_rule(nq) if rule is None else rule
    idx = np.arange(count) if order is None else np.asarray(order)
    out = {"l2": np.zeros(K, T), "h1": np.zeros(K, T)}
    if per_cell:
        out["cell_l2"], out["cell_h1"] = np.zeros((K, count), T), np.zeros((K, count), T)
    if want_points:
        out["points"] = np.empty((count, npts, d), T)
    if samples is not None:
        se = np.asarray(samples[0]).reshape(count, npts)
        sg = None if samples[1] is None else np.asarray(samples[1]).reshape(count, npts, d)
    def one_block(a):
        ids = idx[a:a + block]
        ce = cells[c0 + ids]
        X = coords[ce].astype(T)
        Uc = nodal[:, ce].astype(T)
        xq, uh, gh, wd = _cell_quantities(kind, X, Uc, nq, rule)
        c = ce.shape[0]
        if exact is not None:
            P, G = exact(xq.reshape(-1, d))
            P = P.reshape(-1, c, npts)[fields]
            G = G.reshape(-1, c, npts, d)[fields]
        elif samples is not None:
            P = se[ids].astype(T)[None]
            G = T(0.0) if sg is None else sg[ids].astype(T)[None]
        else:
            P, G = T(0.0), T(0.0)
        l2c = (wd[None] * (uh - P) ** 2).sum(axis=-1)
        h1c = (wd[None] * ((gh - G) ** 2).sum(axis=-1)).sum(axis=-1)
        return ids, l2c, h1c, (xq if want_points else None)

    # the blocks are independent: a few threads evaluate them (NumPy releases the interpreter inside its loops); the
    # results are added in block order, whatever the number of threads
    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        for ids, l2c, h1c, xq in pool.map(one_block, range(0, count, block)):
            out["l2"] += l2c.sum(axis=1)
            out["h1"] += h1c.sum(axis=1)
            if per_cell:
                out["cell_l2"][:, ids], out["cell_h1"][:, ids] = l2c, h1c
            if want_points:
                out["points"][ids] = xq
    if want_points:
        out["points"] = out["points"].reshape(count * npts, d)
    return out


def rel_delta(a64, ald):
    """relative discrepancy of an fp64 result from the longdouble one, entry by entry"""
    ald = np.asarray(ald, np.longdouble)
    return np.asarray(np.abs(np.asarray(a64, np.longdouble) - ald) / np.abs(ald), np.float64)


def norm_bound(delta):
    """the relative bound of a device sum: max(100 delta, 1e-13) (tests/README.md)"""
    return np.maximum(100.0 * np.asarray(delta, np.float64), FLOOR)


# ----------------------------------------------------------------------------------------------------------------------
# Darcy projection
# ----------------------------------------------------------------------------------------------------------------------
def _scatter(idx, w, n):
    if w.dtype == np.float64:
        return np.bincount(idx, weights=w, minlength=n)
    out = np.zeros(n, w.dtype)
    np.add.at(out, idx, w)
    return out


SLABS = 8


def _over_slabs(ncell, block, zeros, add_block):
    """Sums add_block(acc, a, b) over the cell blocks [a, b): the cells are split into SLABS contiguous slabs, each with an
    accumulator of its own (zeros()) filled by one thread; the accumulators are added in slab order, so the result does
    not depend on the number of threads."""
    edges = [ncell * s // SLABS for s in range(SLABS + 1)]

    def one_slab(s):
        acc = zeros()
        for a in range(edges[s], edges[s + 1], block):
            add_block(acc, a, min(a + block, edges[s + 1]))
        return acc

    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        accs = list(pool.map(one_slab, range(SLABS)))
    total = accs[0]
    for acc in accs[1:]:
        total += acc
    return total


def _scatter_add(out, ce, w):
    """out[..., ce[c, b]] += w[..., c, b]; a block of consecutive cells touches a narrow range of nodes"""
    lo, hi = int(ce.min()), int(ce.max()) + 1
    flat = (ce - lo).ravel()
    for i in np.ndindex(*w.shape[:-2]):
        out[i][lo:hi] += _scatter(flat, np.ascontiguousarray(w[i]).ravel(), hi - lo)


def darcy_rhs(kind, cells, coords, p, conductivity, block=1 << 16, longdouble=False):
    """b [K, d, n], b[k, e, a] = int -conductivity (d p_k / d x_e) phi_a for the nodal pressures p [K, n]: 2-point Gauss
    per direction on multilinear cells, the one-point formula on simplices (constant gradient)."""
    T = np.longdouble if longdouble else np.float64
    d = dim_of(kind)
    p = np.atleast_2d(np.asarray(p, dtype=np.float64))
    K, n = p.shape
    kc = T(conductivity)

    def add_block(acc, a, b):
        ce = cells[a:b]
        X = coords[ce].astype(T)
        Pc = p[:, ce].astype(T)
        if kind in (QUAD, HEX):
            xi, w = _tensor_points(2, d, gauss_rule(2), X.dtype)
            N, dN = _multilinear_basis(xi)
            det, I = _det_inv(_jacobian(dN, X))
            g = _matvec(I, _jacobian(dN, Pc[..., None])[..., 0]) * (w[None, :] * np.abs(det))[None, :, :, None]
            contrib = -kc * sum(N[q, None, None, :, None] * g[:, :, q, None, :] for q in range(N.shape[0]))
        else:
            E = X[:, 1:, :] - X[:, :1, :]
            det, I = _det_inv(E)
            g = _matvec(I, Pc[:, :, 1:] - Pc[:, :, :1])
            vol = np.abs(det) / T(2.0 if d == 2 else 6.0)
            contrib = (-kc * vol / T(d + 1))[None, :, None, None] * g[:, :, None, :] * np.ones((1, 1, d + 1, 1), T)
        _scatter_add(acc, ce, np.moveaxis(contrib, 3, 1))      # [K, d, c, nb]

    return _over_slabs(cells.shape[0], block, lambda: np.zeros((K, d, n), T), add_block)


def _element_mass(kind, X):
    """[c, nb, nb] (multilinear: 2-point Gauss per direction) or the factor vol / ((d + 1)(d + 2)) [c] of (1 + I) (simplices)"""
    T = X.dtype.type
    d = X.shape[-1]
    if kind in (QUAD, HEX):
        xi, w = _tensor_points(2, d, gauss_rule(2), X.dtype)
        N, dN = _multilinear_basis(xi)
        det, _ = _det_inv(_jacobian(dN, X))
        wd = w[None, :] * np.abs(det)
        return sum(wd[:, q, None, None] * (N[q, :, None] * N[q, None, :])[None] for q in range(N.shape[0]))
    det, _ = _det_inv(X[:, 1:, :] - X[:, :1, :])
    return np.abs(det) / T((2.0 if d == 2 else 6.0) * (d + 1) * (d + 2))


def mass_apply(kind, cells, coords, x, block=1 << 16, longdouble=False):
    """(M x [K, n], diagonal of M [n]) of the CG-1 mass matrix, cell by cell (no assembled matrix)"""
    T = np.longdouble if longdouble else np.float64
    x = np.atleast_2d(np.asarray(x))
    K, n = x.shape

    def add_block(acc, a, b):
        ce = cells[a:b]
        Me = _element_mass(kind, coords[ce].astype(T))
        xe = x[:, ce].astype(T)
        if Me.ndim == 3:
            ye = sum(Me[None, :, :, j] * xe[:, :, None, j] for j in range(Me.shape[-1]))
            de = np.stack([Me[:, j, j] for j in range(Me.shape[-1])], axis=1)
        else:
            ye = Me[None, :, None] * (xe.sum(axis=-1, keepdims=True) + xe)
            de = np.repeat((2 * Me)[:, None], ce.shape[1], axis=1)
        _scatter_add(acc, ce, np.concatenate([ye, de[None]], axis=0))

    yD = _over_slabs(cells.shape[0], block, lambda: np.zeros((K + 1, n), T), add_block)
    return yD[:K], yD[K]


def mass_1d_banded(nc):
    """the P1 mass matrix of nc equal cells on [0, 1] in the banded storage of scipy.linalg.solve_banded"""
    h = 1.0 / nc
    ab = np.zeros((3, nc + 1))
    ab[1] = 2.0 * h / 3.0
    ab[1, 0] = ab[1, -1] = h / 3.0
    ab[0, 1:] = ab[2, :-1] = h / 6.0
    return ab


def kron_mass_solve(ncells, b):
    """M^-1 b for the Q1 mass matrix of the uniform box with ncells = (nx, ny[, nz]) cells: M is the Kronecker product of
    the 1D P1 mass matrices (x fastest), so one banded solve along each axis; b [K, n] -> [K, n]"""
    b = np.atleast_2d(np.asarray(b, dtype=np.float64))
    shape = tuple(nc + 1 for nc in reversed(ncells))       # [pz,] py, px
    B = b.reshape((b.shape[0],) + shape)
    for ax, nc in enumerate(reversed(ncells)):
        Bm = np.moveaxis(B, ax + 1, 0)
        sol = sla.solve_banded((1, 1), mass_1d_banded(nc), np.ascontiguousarray(Bm).reshape(nc + 1, -1))
        B = np.moveaxis(sol.reshape(Bm.shape), 0, ax + 1)
    return np.ascontiguousarray(B).reshape(b.shape)


def dnorm(D, r):
    """||D^-1 r||_2 per leading index"""
    q = np.asarray(r) / D
    return np.sqrt((q * q).sum(axis=-1))


def diag_ratio(D):
    return float(D.max() / D.min())


def error_factor(kind, D):
    """c with ||M^-1 r||_2 <= c ||D^-1 r||_2: M^-1 r = D^-1/2 S^-1 D^1/2 (D^-1 r) with S = D^-1/2 M D^-1/2, whose smallest
    eigenvalue is that of D^-1 M, so c = sqrt(max D / min D) / lambda_min"""
    return float(np.sqrt(diag_ratio(D)) / LAMBDA_MIN[kind])


def residual_drift(kind, cells, coords, p, conductivity, u):
    """The reference's own residual-evaluation drift: ||D^-1 (r_64 - r_ld)||_2 / ||D^-1 b||_2, largest over the
    components, where r = b - M u is evaluated wholly (right-hand side and product) in fp64 and in np.longdouble;
    p [n], u [d, n]"""
    r = []
    for ld in (False, True):
        b = darcy_rhs(kind, cells, coords, p, conductivity, longdouble=ld)[0]
        y, D = mass_apply(kind, cells, coords, u, longdouble=ld)
        r.append((b - y, b, D))
    (r64, _, _), (rld, bld, Dld) = r
    return float(np.max(dnorm(Dld, np.asarray(r64, np.longdouble) - rld) / dnorm(Dld, bld)))


def projection_bound(kind, D, b, drift, rtol=CG_RTOL):
    """(bound on ||D^-1 (b - M u)||_2, bound on ||u - M^-1 b||_2) per leading index of b, for a u whose solver stopped at
    ||D^-1 r||_2 <= rtol ||D^-1 b||_2, checked with a residual whose own evaluation drifts by `drift`"""
    res = (rtol + 100.0 * drift) * dnorm(D, b)
    return res, error_factor(kind, D) * res


# ----------------------------------------------------------------------------------------------------------------------
# the cases of test_post_scale_gpu.py (test_post_scale_host.py asserts the side of the threshold each one is on) and
# the comparisons it makes (test_post_scale_host.py feeds them wrong results)
# ----------------------------------------------------------------------------------------------------------------------
K1, K2, BETA, MU = 1.0, 0.01, 1.0, 1.0
CONDUCTIVITY = 0.37
NORM_PAST = {"quad800x700": (QUAD, 800, 700, 0), "quad1024x513": (QUAD, 1024, 513, 0), "tri600x500": (TRI, 600, 500, 0),
             "hex84x80x80": (HEX, 84, 80, 80), "tet48x48x40": (TET, 48, 48, 40)}
NORM_AT = {"quad1024x512": (QUAD, 1024, 512, 0)}
NORM_SMALL = {"quad12x9": (QUAD, 12, 9, 0), "tri12x9": (TRI, 12, 9, 0), "hex12x9x5": (HEX, 12, 9, 5), "tet6x5x4": (TET, 6, 5, 4)}
DARCY_PAST = {"quad1500x1400": (QUAD, 1500, 1400, 0), "tri1500x1400": (TRI, 1500, 1400, 0),
              "hex128x128x127": (HEX, 128, 128, 127), "tet128x128x127": (TET, 128, 128, 127)}
DARCY_SMALL = {"hex37x5x11": (HEX, 37, 5, 11), "tet9x14x6": (TET, 9, 14, 6), "quad61x47": (QUAD, 61, 47, 0),
               "tri53x41": (TRI, 53, 41, 0), "quad16x15": (QUAD, 16, 15, 0),
               "quad1x1": (QUAD, 1, 1, 0), "quad2x2": (QUAD, 2, 2, 0), "tri1x1": (TRI, 1, 1, 0), "tri2x2": (TRI, 2, 2, 0),
               "hex1x1x1": (HEX, 1, 1, 1), "hex2x2x2": (HEX, 2, 2, 2), "tet1x1x1": (TET, 1, 1, 1), "tet2x2x2": (TET, 2, 2, 2)}
# the mesh of each kind on which the residual-evaluation drift is measured
DRIFT_MESH = {QUAD: "quad61x47", TRI: "tri53x41", HEX: "hex37x5x11", TET: "tet9x14x6"}
LINEAR_A = np.array([0.5, -1.25, 2.0])


def norm_fields(X):
    """(nodal [4, n], fields [4], exact): the interpolants of both manufactured pressures times 1 + 0.1 s(x) (errors of
    order 0.1: a well-conditioned sum), then the plain interpolants (errors of order h^2: the cancellation case)"""
    ex = mms_exact(X.shape[1], K1, K2, BETA, MU)
    P, _ = ex(X)
    fac = smooth_factor(X)
    return np.stack([P[0] * fac, P[1] * fac, P[0], P[1]]), np.array([0, 1, 0, 1]), ex


NODAL_NAME = ("p1 (1 + 0.1 s)", "p2 (1 + 0.1 s)", "interpolant of p1", "interpolant of p2")


def threaded(f, pieces=8):
    """f: X [m, d] -> array with leading m, evaluated in `pieces` row blocks on the thread pool"""
    def g(X):
        edges = [X.shape[0] * s // pieces for s in range(pieces + 1)]
        with ThreadPoolExecutor(max_workers=WORKERS) as pool:
            return np.concatenate(list(pool.map(lambda s: f(X[edges[s]:edges[s + 1]]), range(pieces))), axis=0)
    return g


def norm_reference(kind, cells, X, nq):
    """fp64 sums, their relative bounds max(100 delta, 1e-13) with delta against np.longdouble, and delta itself"""
    nodal, fields, ex = norm_fields(X)
    r64 = error_sums(kind, cells, X, nodal, fields, nq, exact=ex)
    rld = error_sums(kind, cells, X, nodal, fields, nq, exact=ex, longdouble=True)
    delta = {s: rel_delta(r64[s], rld[s]) for s in ("l2", "h1")}
    return {"nodal": nodal, "fields": fields, "exact": ex, "l2": r64["l2"], "h1": r64["h1"], "delta": delta,
            "bound": {s: norm_bound(delta[s]) for s in ("l2", "h1")}}


def norms_excess(ref, k, l2sq, h1sq):
    """largest |got - ref| / (bound ref) over the two squared sums of nodal field k: the comparison passes at <= 1"""
    return max(abs(l2sq - ref["l2"][k]) / (ref["bound"]["l2"][k] * ref["l2"][k]),
               abs(h1sq - ref["h1"][k]) / (ref["bound"]["h1"][k] * ref["h1"][k]))


def points_bound(kind, xmax):
    """|x_q - x_q,ref| elementwise: either evaluation rounds each of the nb products N_b x_b and their sum, and N_b (or the
    simplex's edge vectors and barycentric weights) in at most 3 d + 2 operations: 2 (nb + 3 d + 2) u max |x|"""
    d = dim_of(kind)
    nb = (1 << d) if kind in (QUAD, HEX) else d + 1
    return 2.0 * (nb + 3 * d + 2) * U * xmax


def points_excess(kind, xq, xref):
    return float(np.abs(xq - xref).max() / points_bound(kind, float(np.abs(xref).max())))


def quadrature_points(kind, cells, X, nq, cell_range):
    return error_sums(kind, cells, X, np.zeros((1, X.shape[0])), [0], nq, cell_range=cell_range, want_points=True)["points"]


def darcy_pressures(X, seed=11):
    """a random nodal pressure and a linear one (whose projection is the constant -conductivity a)"""
    d = X.shape[1]
    return np.stack([np.random.default_rng(seed).standard_normal(X.shape[0]), X @ LINEAR_A[:d] + 3.0])


def darcy_excess(kind, cells, X, p, u, drift, direct=None, b=None):
    """The comparisons of a projection u [K, d, n] of the pressures p [K, n] (p[-1] linear): residual r = b_ref - M u in the
    D^-1 norm, distance from the constant for the linear pressure, distance from the direct solves direct [K, d, n]
    (whose own error is bounded through their residual) - each divided by its bound.  Returns (dict of excesses,
    dict of figures)."""
    d = dim_of(kind)
    K, n = p.shape
    b = (darcy_rhs(kind, cells, X, p, CONDUCTIVITY) if b is None else np.asarray(b)).reshape(K * d, n)
    u = np.asarray(u).reshape(K * d, n)
    y, D = mass_apply(kind, cells, X, u)
    bres, berr = projection_bound(kind, D, b, drift)
    res = dnorm(D, b - y)
    exc = {"residual": float(np.max(res / bres))}
    fig = {"ratio": diag_ratio(D), "factor": error_factor(kind, D), "res": float(np.max(res / dnorm(D, b))),
           "res_bound": CG_RTOL + 100.0 * drift}
    const = -CONDUCTIVITY * LINEAR_A[:d]
    elin = np.sqrt(((u[(K - 1) * d:] - const[:, None]) ** 2).sum(axis=1))
    exc["linear"] = float(np.max(elin / berr[(K - 1) * d:]))
    fig["linear"] = float(np.max(elin))
    fig["linear_bound"] = float(np.min(berr[(K - 1) * d:]))
    if direct is not None:
        direct = np.asarray(direct).reshape(K * d, n)
        yd, _ = mass_apply(kind, cells, X, direct)
        own = error_factor(kind, D) * dnorm(D, b - yd)
        dist = np.sqrt(((u - direct) ** 2).sum(axis=1))
        exc["direct"] = float(np.max(dist / (berr + own)))
        fig["direct"] = float(np.max(dist / np.sqrt((direct ** 2).sum(axis=1))))
    return exc, fig
