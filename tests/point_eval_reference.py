"""NumPy restatement of point evaluation (Function.at / gradient_at) in np.longdouble, written from the documented
conventions (include/perphil_hip.h, perphil_amd/csrc/pph_p2.h), not from the kernel.  No tests in here.

Geometry is the EXACT uniform lattice: node id -> lattice index -> index / (degree * n) in longdouble (the double
coordinates of the mesh arrays are themselves rounded and are not used).

`evaluate` locates every point by brute force over the `cells` array (oracle.build_mesh for CG-1, p2_restatement.dofmap
for degree 2): reference coordinates of the point in every cell from the cell's frame vertices, the first cell that
contains it gives value and gradient.  `evaluate_fast` is the vectorised variant for millions of points: box by floor,
sub-cell = the lowest index whose barycentric coordinates are all >= 0, node ids by lattice arithmetic.

Both return, per point and component, beside value `v` and physical gradient `g`:
  S      = sum_b |N_b| |u_b|
  G[e]   = sum_b |d N_b / d xi_e| |u_b|             (xi: box-local coordinates, x_e = (c_e + xi_e) / n_e)
  H[e,f] = sum_b |d2 N_b / d xi_e d xi_f| |u_b|
In `evaluate` S, G, H are the maxima over ALL cells that contain the point to within `face_tol` box-local units: the
one rounding of x_e n_e in double can carry a point across a face, and the Lipschitz bounds built from G and H must
then hold on both sides.  Points outside the unit box by no more than `tol` box-local units are clamped onto it first,
as the documented location rule does."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2_restatement as p2r  # noqa: E402

LD = np.longdouble
QUAD, TRI, HEX, TET = 0, 1, 2, 3
U = LD(2.0) ** -53


def dim_of(kind):
    return 2 if kind in (QUAD, TRI) else 3


def boxes(kind, nx, ny, nz=0):
    return np.array([nx, ny, nz][: dim_of(kind)], dtype=np.int64)


def cells_of(kind, degree, nx, ny, nz=0):
    if degree == 2:
        return p2r.dofmap(kind, nx, ny, nz)
    from oracle import dpp_oracle as o

    return o.build_mesh(dim_of(kind), kind, nx, ny, nz).cells


def n_nodes(kind, degree, nx, ny, nz=0):
    return int(np.prod(degree * boxes(kind, nx, ny, nz) + 1))


def lattice_index(ids, kind, degree, nx, ny, nz=0):
    d = dim_of(kind)
    p = degree * boxes(kind, nx, ny, nz) + 1
    ids = np.asarray(ids, dtype=np.int64)
    cols = [ids % p[0], (ids // p[0]) % p[1]]
    if d == 3:
        cols.append(ids // (p[0] * p[1]))
    return np.stack(cols, axis=-1)


def node_coords(ids, kind, degree, nx, ny, nz=0):
    """Exact lattice coordinates (longdouble) of node ids."""
    return lattice_index(ids, kind, degree, nx, ny, nz).astype(LD) / (degree * boxes(kind, nx, ny, nz)).astype(LD)


def frame_locals(kind, degree):
    if degree == 2:
        return p2r.frame_locals(kind)
    return {QUAD: [0, 1, 2], HEX: [0, 1, 2, 4], TRI: [0, 1, 2], TET: [0, 1, 2, 3]}[kind]


# ---------------------------------------------------------------------------------------------------------------
# reference bases, vectorised over points: N [P, m], G [P, m, d], H [P, m, d, d] in reference coordinates
# ---------------------------------------------------------------------------------------------------------------
def _l1(deg, i, t):
    one = np.ones_like(t)
    if deg == 1:
        return ((1 - t, -one, 0 * one), (t, one, 0 * one))[i]
    return (((2 * t - 1) * (t - 1), 4 * t - 3, 4 * one), (4 * t * (1 - t), 4 - 8 * t, -8 * one),
            (t * (2 * t - 1), 4 * t - 1, 4 * one))[i]


def basis_all(kind, degree, R, hess=True):
    R = np.asarray(R, dtype=LD)
    P, d = R.shape
    if kind in (QUAD, HEX):
        k = degree + 1
        m = k ** d
        N = np.empty((P, m), LD); G = np.empty((P, m, d), LD); H = np.empty((P, m, d, d) if hess else (0,), LD)
        for a in range(m):
            ia = [a % k, (a // k) % k, a // (k * k)][:d]
            f = [_l1(degree, ia[e], R[:, e]) for e in range(d)]

            def prod(orders):
                out = np.ones(P, LD)
                for e in range(d):
                    out = out * f[e][orders[e]]
                return out
            N[:, a] = prod([0] * d)
            for e in range(d):
                G[:, a, e] = prod([1 if q == e else 0 for q in range(d)])
                for g in range(d if hess else 0):
                    H[:, a, e, g] = prod([(1 if q == e else 0) + (1 if q == g else 0) for q in range(d)])
        return N, G, H
    lam = np.concatenate([(1 - R.sum(axis=1))[:, None], R], axis=1)
    dl = np.vstack([-np.ones(d), np.eye(d)]).astype(LD)
    if degree == 1:
        return lam, np.broadcast_to(dl, (P, d + 1, d)).copy(), np.zeros((P, d + 1, d, d), LD)
    E = p2r.TRI_E if kind == TRI else p2r.TET_E
    m = d + 1 + len(E)
    N = np.empty((P, m), LD); G = np.empty((P, m, d), LD); H = np.empty((P if hess else 0, m, d, d), LD)
    for r in range(d + 1):
        N[:, r] = lam[:, r] * (2 * lam[:, r] - 1)
        G[:, r] = (4 * lam[:, r] - 1)[:, None] * dl[r]
        H[:, r] = 4 * np.outer(dl[r], dl[r])
    for i, (p, q) in enumerate(E):
        N[:, d + 1 + i] = 4 * lam[:, p] * lam[:, q]
        G[:, d + 1 + i] = 4 * (lam[:, q][:, None] * dl[p] + lam[:, p][:, None] * dl[q])
        H[:, d + 1 + i] = 4 * (np.outer(dl[p], dl[q]) + np.outer(dl[q], dl[p]))
    return N, G, H


def _inverse_ld(J):
    """Inverses of [C, d, d] longdouble matrices by the adjugate."""
    d = J.shape[-1]
    if d == 2:
        det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
        adj = np.stack([np.stack([J[:, 1, 1], -J[:, 0, 1]], -1), np.stack([-J[:, 1, 0], J[:, 0, 0]], -1)], -2)
        return adj / det[:, None, None]
    c = np.empty_like(J)
    for i in range(3):
        for j in range(3):
            r = [q for q in range(3) if q != i]
            s = [q for q in range(3) if q != j]
            c[:, i, j] = (-1) ** (i + j) * (J[:, r[0], s[0]] * J[:, r[1], s[1]] - J[:, r[0], s[1]] * J[:, r[1], s[0]])
    det = (J[:, 0, :] * c[:, 0, :]).sum(axis=1)
    return np.transpose(c, (0, 2, 1)) / det[:, None, None]


def clamp_points(pts, n, tol):
    """Points (longdouble) outside the unit box by at most tol box-local units, clamped onto it; [P] bool: outside."""
    X = np.asarray(pts).astype(LD)
    t = X * n.astype(LD)
    outside = np.any((t < -LD(tol)) | (t - n.astype(LD) > LD(tol)) | np.isnan(t), axis=1)
    return np.clip(X, LD(0), LD(1)), outside


def evaluate(kind, degree, nx, ny, nz, u, pts, tol=1e-12, face_tol=None):
    """Brute force over the cells array.  u: [n] or [n, ncomp]; pts: [P, d] doubles.  Outside points give NaN."""
    d = dim_of(kind)
    n = boxes(kind, nx, ny, nz)
    nl = n.astype(LD)
    cells = cells_of(kind, degree, nx, ny, nz)
    u = np.asarray(u, dtype=np.float64).reshape(n_nodes(kind, degree, nx, ny, nz), -1).astype(LD)
    nc = u.shape[1]
    if face_tol is None:
        face_tol = float(2.0 ** -50 * n.max())
    fr = frame_locals(kind, degree)
    X0 = node_coords(cells[:, fr[0]], kind, degree, nx, ny, nz)                                  # [C, d]
    J = np.stack([node_coords(cells[:, fr[j + 1]], kind, degree, nx, ny, nz) - X0 for j in range(d)], axis=-1)   # columns
    Ji = _inverse_ld(J)                                                                         # [C, d(ref j), d(phys e)]
    X, outside = clamp_points(pts, n, tol)
    P = X.shape[0]
    simplex = kind in (TRI, TET)
    out = dict(v=np.full((P, nc), np.nan, LD), g=np.full((P, nc, d), np.nan, LD), S=np.zeros((P, nc), LD),
               G=np.zeros((P, nc, d), LD), H=np.zeros((P, nc, d, d), LD), cell=np.full(P, -1, np.int64), outside=outside)
    eps = LD(2.0) ** -58
    for k in range(P):
        if outside[k]:
            continue
        R = np.einsum("cje,ce->cj", Ji, X[k] - X0)                                              # ref coords in every cell
        # slack of the containment inequalities in BOX-LOCAL units (ref coords of all four kinds are box-local lengths)
        slack = np.minimum(R.min(axis=1), (1 - R.sum(axis=1)) if simplex else (1 - R).min(axis=1))
        first = int(np.argmax(slack >= -eps))
        assert slack[first] >= -eps, f"point {pts[k]} found in no cell"
        for c in np.nonzero(slack >= -LD(face_tol))[0]:
            Rc = R[c:c + 1]
            if degree == 2 and c == first:
                Nn, Gg = p2r.basis(kind, R[c])
                N, Gr, Hr = Nn[None], Gg[None], basis_all(kind, degree, Rc)[2]
            else:
                N, Gr, Hr = basis_all(kind, degree, Rc)
            N, Gr, Hr = N[0], Gr[0], Hr[0]
            gp = Gr @ Ji[c]                                       # [m, e] physical gradients of the basis
            hp = np.einsum("bjk,je,kf->bef", Hr, Ji[c], Ji[c])
            ub = u[cells[c]]                                      # [m, nc]
            au = np.abs(ub)
            if c == first:
                out["v"][k] = N @ ub
                out["g"][k] = np.einsum("be,bc->ce", gp, ub)
                out["cell"][k] = c
            out["S"][k] = np.maximum(out["S"][k], np.abs(N) @ au)
            out["G"][k] = np.maximum(out["G"][k], np.einsum("be,bc->ce", np.abs(gp), au) / nl)
            out["H"][k] = np.maximum(out["H"][k], np.einsum("bef,bc->cef", np.abs(hp), au) / (nl[:, None] * nl[None, :]))
    return out


# ---------------------------------------------------------------------------------------------------------------
# vectorised variant
# ---------------------------------------------------------------------------------------------------------------
def _subcell_tables(kind, degree):
    """Per sub-cell s: A[s] with lam = A[s] @ [1, xi] (barycentric coordinates of the sub-cell's local vertices, from its
    corner list alone) and off[s][b] = lattice offset (units of the degree-`degree` lattice) of local node b in the box."""
    d = dim_of(kind)
    if kind in (QUAD, HEX):
        k = degree + 1
        off = [[[a % k, (a // k) % k, a // (k * k)][:d] for a in range(k ** d)]]
        return None, np.array(off, dtype=np.int64)
    V = p2r.TRI_V if kind == TRI else p2r.TET_V
    A, off = [], []
    for s, verts in enumerate(V):
        C = np.array([[1.0] + [(v >> e) & 1 for e in range(d)] for v in verts])      # lam(corner_q) = delta
        A.append(np.rint(np.linalg.inv(C).T))
        if degree == 2:
            off.append([o[:d] for o in p2r.local_offsets(kind, s)])
        else:
            off.append([[(v >> e) & 1 for e in range(d)] for v in verts])
    return np.array(A), np.array(off, dtype=np.int64)


def locate_fast(kind, nx, ny, nz, pts, tol=1e-12):
    """Box index per direction [P, d], box-local coordinates (longdouble, clamped) and outside flags, by the documented
    rule in longdouble (no rounding of x n to double)."""
    n = boxes(kind, nx, ny, nz)
    X, outside = clamp_points(pts, n, tol)
    X = np.where(np.isnan(X), LD(0), X)          # (outside; kept finite so that the indexing below stays in range)
    t = X * n.astype(LD)
    c = np.clip(np.floor(t), 0, (n - 1).astype(LD))
    return c.astype(np.int64), t - c, outside


def face_distance(kind, nx, ny, nz, pts):
    """Smallest distance (box-local units, unnormalised for the diagonal planes) of each point to a cell or sub-cell face."""
    _, xi, _ = locate_fast(kind, nx, ny, nz, pts)
    d = np.minimum(xi.min(axis=1), (1 - xi).min(axis=1))
    if kind == TRI:
        d = np.minimum(d, np.abs(xi[:, 0] + xi[:, 1] - 1))
    if kind == TET:
        for a, b in ((0, 1), (0, 2), (1, 2)):
            d = np.minimum(d, np.abs(xi[:, a] - xi[:, b]))
    return d.astype(np.float64)


def evaluate_fast(kind, degree, nx, ny, nz, u, pts, tol=1e-12, gradient=True, chunk=1 << 17):
    d = dim_of(kind)
    n = boxes(kind, nx, ny, nz)
    nl = n.astype(LD)
    u = np.asarray(u, dtype=np.float64).reshape(n_nodes(kind, degree, nx, ny, nz), -1)
    nc = u.shape[1]
    A, off = _subcell_tables(kind, degree)
    p = degree * n + 1
    P = len(pts)
    out = dict(v=np.full((P, nc), np.nan, LD), S=np.zeros((P, nc), LD), G=np.zeros((P, nc, d), LD),
               outside=np.zeros(P, bool), sub=np.zeros(P, np.int64))
    if gradient:
        out["g"] = np.full((P, nc, d), np.nan, LD)
        out["H"] = np.zeros((P, nc, d, d), LD)
    for b0 in range(0, P, chunk):
        sl = slice(b0, min(P, b0 + chunk))
        c, xi, outside = locate_fast(kind, nx, ny, nz, pts[sl], tol)
        Q = xi.shape[0]
        if A is None:
            sub = np.zeros(Q, np.int64)
            R = xi
            D = np.broadcast_to(np.eye(d), (Q, d, d))
        else:
            h = np.concatenate([np.ones((Q, 1), LD), xi], axis=1)
            lam_all = np.einsum("srk,pk->psr", A.astype(LD), h)                     # [Q, s, r]
            sub = np.argmax((lam_all >= 0).all(axis=2), axis=1)                       # lowest index that contains the point
            lam = lam_all[np.arange(Q), sub]
            R = lam[:, 1:]
            D = A[sub][:, 1:, 1:]                                                     # d ref_j / d xi_e
        N, Gr, Hr = basis_all(kind, degree, R, hess=gradient)
        Dl = D.astype(LD)
        gx = np.einsum("pbj,pje->pbe", Gr, Dl)                                        # box-local derivatives
        base = degree * c                                                             # [Q, d]
        lat = base[:, None, :] + off[sub]                                             # [Q, m, d]
        node = lat[..., 0] + p[0] * lat[..., 1]
        if d == 3:
            node = node + p[0] * p[1] * lat[..., 2]
        ub = u[node].astype(LD)                                                       # [Q, m, nc]
        au = np.abs(ub)
        v = np.einsum("pb,pbc->pc", N, ub)
        v[outside] = np.nan
        out["v"][sl] = v
        out["S"][sl] = np.einsum("pb,pbc->pc", np.abs(N), au)
        out["G"][sl] = np.einsum("pbe,pbc->pce", np.abs(gx), au)
        out["outside"][sl] = outside
        out["sub"][sl] = sub
        if gradient:
            g = np.einsum("pbe,pbc->pce", gx, ub) * nl
            g[outside] = np.nan
            out["g"][sl] = g
            hx = np.einsum("pbjk,pje,pkf->pbef", Hr, Dl, Dl)
            out["H"][sl] = np.einsum("pbef,pbc->pcef", np.abs(hx), au)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the bounds of the GPU tests
# ---------------------------------------------------------------------------------------------------------------
# gamma: roundings on the longest path from the box-local coordinates xi (exact: xi = t - c) to an output, per
# (kind, degree), counted on the expressions of pph_eval.hip / pph_p2.h without assuming any fused multiply-add:
#   Q1: w = 1 - xi (1), N = w w (w) (d - 1), product N u (1), sum of 2^d terms (2^d - 1):       d + 2^d
#   P1: lam: at most 2 subtractions (2), product (1), sum of d + 1 terms (d):                    3 + d
#   Q2: 1-D factor (2t - 1)(t - 1) (3), N = v v (v) (3 d + d - 1), product (1), sum (3^d - 1):   4 d - 1 + 3^d
#   P2: reference coordinates (2), lam_0 = 1 - sum (d) -> lam: 2 + d; N = lam (2 lam - 1): 2 (2 + d) + 2, product (1),
#       sum of m terms (m - 1):                                                                  6 + 2 d + m
# plus 1 for the second-order terms of (1 + 2^-53)^gamma and the longdouble reference's own rounding.
# Differences such as 1 - xi_x - xi_y cancel, so their error is absolute rather than relative to the result; xi is a
# multiple of 2^-52 outside the first box of a direction, where those differences are therefore exact, and inside the first
# box (t_e = xi_e) the absolute error 2^-54 of a difference is covered by the part of the xi term, 2^-53 n_e G_e, that the
# rounding of x_e n_e (at most 2^-53 xi_e n_e there) does not use when xi_e < 1/2, while for xi_e >= 1/2 the difference
# 1 - xi_e is exact (Sterbenz).
def gamma_value(kind, degree):
    d = dim_of(kind)
    if degree == 1:
        return (d + 2 ** d if kind in (QUAD, HEX) else 3 + d) + 1
    m = p2r.nodes_per_cell(kind)
    return (4 * d - 1 + 3 ** d if kind in (QUAD, HEX) else 6 + 2 * d + m) + 1


# gradient: no derivative of a basis function takes more roundings than the function itself; the chain rule to the box's
# axes adds d - 1 additions (simplices), the scaling by n_e one more rounding.
def gamma_gradient(kind, degree):
    return gamma_value(kind, degree) + dim_of(kind)


def value_bound(kind, degree, nx, ny, nz, ref):
    """[P, nc]: 2^-53 (gamma S + sum_e n_e G_e)."""
    nl = boxes(kind, nx, ny, nz).astype(LD)
    return U * (gamma_value(kind, degree) * ref["S"] + (ref["G"] * nl).sum(axis=-1))


def gradient_bound(kind, degree, nx, ny, nz, ref):
    """[P, nc, d]: 2^-53 n_e (gamma_g G_e + sum_f n_f H_ef) for the physical gradient n_e d/d xi_e."""
    nl = boxes(kind, nx, ny, nz).astype(LD)
    return U * nl * (gamma_gradient(kind, degree) * ref["G"] + (ref["H"] * nl).sum(axis=-1))


# ---------------------------------------------------------------------------------------------------------------
# the inputs the host and GPU tests share (same seeds on both sides)
# ---------------------------------------------------------------------------------------------------------------
CASES = [(QUAD, 7, 5, 0), (TRI, 7, 5, 0), (HEX, 5, 4, 3), (TET, 5, 4, 3)]
N_RANDOM = 2000


def case_seed(kind, degree):
    return 1000 + 10 * kind + degree


def random_coefficients(kind, degree, nx, ny, nz, ncomp=1, seed=None):
    """Mixed sign and magnitude: normal deviates times 10^U(-3, 3)."""
    rng = np.random.default_rng(case_seed(kind, degree) + 7 if seed is None else seed)
    n = n_nodes(kind, degree, nx, ny, nz)
    return rng.standard_normal((n, ncomp)) * 10.0 ** rng.uniform(-3, 3, (n, ncomp))


def random_points(kind, degree, count=N_RANDOM):
    return np.random.default_rng(case_seed(kind, degree)).random((count, dim_of(kind)))


def deliberate_points(kind, nx, ny, nz=0, seed=5):
    """Domain corners, cell vertices, edge / face midpoints (the lattice refined once), points on box faces, on the triangle
    diagonal and the Kuhn interior faces, and points within 1e-13 box-local units of a face on either side (the domain's
    own faces included: those 1e-13 outside are inside by the default tolerance 1e-12)."""
    import itertools

    d = dim_of(kind)
    n = boxes(kind, nx, ny, nz)
    rng = np.random.default_rng(seed)
    out = [np.array(list(itertools.product((0.0, 1.0), repeat=d)))]
    out.append(np.array(list(itertools.product(*[np.arange(2 * n[e] + 1) / (2 * n[e]) for e in range(d)]))))
    for e in range(d):                      # on the box faces normal to e, and 1e-13 to either side
        for i in range(n[e] + 1):
            X = rng.random((6, d))
            for delta in (0.0, -1e-13, 1e-13):
                Y = X.copy()
                Y[:, e] = (i + delta) / n[e]
                out.append(Y)
    if kind in (TRI, TET):                  # sub-cell faces inside random boxes
        for _ in range(60):
            c = np.array([rng.integers(0, n[e]) for e in range(d)])
            xi = rng.random(d)
            if kind == TRI:
                faces = [np.array([xi[0], 1 - xi[0]])]
            else:
                a, b, cc = xi
                faces = [np.array([a, a, cc]), np.array([a, b, a]), np.array([a, b, b]), np.array([a, a, a])]
            for f in faces:
                for delta in (0.0, -1e-13, 1e-13):
                    g = f.copy()
                    g[0] = min(max(g[0] + delta, 0.0), 1.0)
                    out.append(((c + g) / n)[None])
    return np.concatenate(out, axis=0)


def integer_polynomial(kind, degree, nx, ny, nz=0):
    """A polynomial the space holds exactly, with integer values at the nodes (so the interpolant's coefficients carry no
    rounding): in the lattice coordinates T_e = degree n_e x_e, degree 1: affine (simplices) / multilinear, degree 2: a
    full quadratic.  Returns f(T) for longdouble or float arrays T [P, d]."""
    d = dim_of(kind)

    def f(T):
        x, y = T[:, 0], T[:, 1]
        z = T[:, 2] if d == 3 else 0 * x
        if degree == 1 and kind in (TRI, TET):
            return 3 + 2 * x - 5 * y + 7 * z
        if degree == 1:
            return 3 + 2 * x - 5 * y + 7 * z + 4 * x * y - 3 * y * z + 2 * x * z + (x * y * z if d == 3 else 0)
        return 3 + 2 * x - 5 * y + 7 * z + 4 * x * y - 3 * y * z + 2 * x * z + 3 * x * x - 2 * y * y + z * z
    return f
