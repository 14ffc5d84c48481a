"""NumPy / SciPy restatement of the degree-2 (Q2 / P2) discretisation on the structured meshes, for small meshes: lattice
numbering, cell->dof map, element matrices by high-order quadrature, global K / M, Dirichlet elimination into the DPP
blocks, and IKJ ILU(0) + GMRES(30) for iteration counts.  Written from the documented conventions
(include/perphil_hip.h, perphil_amd/csrc/pph_p2.h), independently of the library's code.

Lattice: node (I,J,K) -> I + (2nx+1)(J + (2ny+1)K) at (I/2nx, J/2ny, K/2nz).
Local order: Q2 -> lattice offset (a,b,c) of the box, local a + 3b + 9c; P2 -> the CG-1 vertices of the cell (vertex
order of the CG-1 dof map), then the edge midpoints 01, 02, 12 (triangles) / 01, 02, 03, 12, 13, 23 (tetrahedra)."""
from __future__ import annotations

import itertools

import numpy as np
import scipy.sparse as sp

QUAD, TRI, HEX, TET = 0, 1, 2, 3
TRI_V = [(0, 1, 2), (1, 3, 2)]          # CG-1 vertices (box corner v = x + 2y + 4z) of the sub-cells of a box
TET_V = [(0, 1, 3, 7), (0, 1, 7, 5), (0, 5, 7, 4), (0, 3, 2, 7), (0, 6, 4, 7), (0, 2, 6, 7)]
TRI_E = [(0, 1), (0, 2), (1, 2)]
TET_E = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def dim_of(kind):
    return 2 if kind in (QUAD, TRI) else 3


def nodes_per_cell(kind):
    return {QUAD: 9, TRI: 6, HEX: 27, TET: 10}[kind]


def cells_per_box(kind):
    return {QUAD: 1, TRI: 2, HEX: 1, TET: 6}[kind]


def lattice_dims(kind, nx, ny, nz=0):
    return 2 * nx + 1, 2 * ny + 1, (2 * nz + 1 if dim_of(kind) == 3 else 1)


def n_nodes(kind, nx, ny, nz=0):
    px, py, pz = lattice_dims(kind, nx, ny, nz)
    return px * py * pz


def coords(kind, nx, ny, nz=0):
    px, py, pz = lattice_dims(kind, nx, ny, nz)
    ids = np.arange(px * py * pz)
    cols = [(ids % px) / (2 * nx), ((ids // px) % py) / (2 * ny)]
    if dim_of(kind) == 3:
        cols.append((ids // (px * py)) / (2 * nz))
    return np.stack(cols, axis=1)


def boundary_nodes(kind, nx, ny, nz=0):
    X = coords(kind, nx, ny, nz)
    return np.nonzero(np.any((X == 0.0) | (X == 1.0), axis=1))[0].astype(np.int64)


def _corner(v):
    return np.array([2 * (v & 1), 2 * ((v >> 1) & 1), 2 * ((v >> 2) & 1)])


def local_offsets(kind, s):
    """Lattice offsets inside the box of the local nodes of sub-cell s."""
    r = range(3)
    if kind == QUAD:
        return [np.array([a, b, 0]) for b in r for a in r]
    if kind == HEX:
        return [np.array([a, b, c]) for c in r for b in r for a in r]
    V, E = (TRI_V, TRI_E) if kind == TRI else (TET_V, TET_E)
    verts = [_corner(v) for v in V[s]]
    return verts + [(verts[p] + verts[q]) // 2 for p, q in E]


def dofmap(kind, nx, ny, nz=0):
    px, py, _ = lattice_dims(kind, nx, ny, nz)
    nzb = nz if dim_of(kind) == 3 else 1
    out = []
    for bz, by, bx in itertools.product(range(nzb), range(ny), range(nx)):
        for s in range(cells_per_box(kind)):
            out.append([(2 * bx + o[0]) + px * ((2 * by + o[1]) + py * (2 * bz + o[2])) for o in local_offsets(kind, s)])
    return np.array(out, dtype=np.int32)


def _l1d(i, t):
    return [(2 * t - 1) * (t - 1), 4 * t * (1 - t), t * (2 * t - 1)][i], [4 * t - 3, 4 - 8 * t, 4 * t - 1][i]


def basis(kind, xi):
    """Values [m] and reference gradients [m, d] at one reference point."""
    d = dim_of(kind)
    if kind in (QUAD, HEX):
        N, G = [], []
        for a in range(nodes_per_cell(kind)):
            ia = [a % 3, (a // 3) % 3, a // 9][:d]
            v = [_l1d(ia[e], xi[e]) for e in range(d)]
            N.append(np.prod([x[0] for x in v]))
            G.append([np.prod([v[f][1] if f == e else v[f][0] for f in range(d)]) for e in range(d)])
        return np.array(N), np.array(G)
    lam = np.concatenate([[1 - sum(xi)], xi])
    dl = np.vstack([-np.ones(d), np.eye(d)])
    N = [lam[r] * (2 * lam[r] - 1) for r in range(d + 1)]
    G = [(4 * lam[r] - 1) * dl[r] for r in range(d + 1)]
    for p, q in (TRI_E if kind == TRI else TET_E):
        N.append(4 * lam[p] * lam[q])
        G.append(4 * (dl[p] * lam[q] + lam[p] * dl[q]))
    return np.array(N), np.array(G)


def reference_rule(kind, n=6):
    """n-point Gauss per direction on [0,1]^d, collapsed onto the simplex: far beyond the degree-4 integrands."""
    x, w = np.polynomial.legendre.leggauss(n)
    x, w = 0.5 * (x + 1), 0.5 * w
    d = dim_of(kind)
    pts, wts = [], []
    for idx in itertools.product(range(n), repeat=d):
        if kind in (QUAD, HEX):
            pts.append([x[i] for i in idx])
            wts.append(np.prod([w[i] for i in idx]))
            continue
        u, v = x[idx[0]], x[idx[1]]
        if d == 2:
            pts.append([u, v * (1 - u)])
            wts.append(w[idx[0]] * w[idx[1]] * (1 - u))
        else:
            t = x[idx[2]]
            pts.append([u, v * (1 - u), t * (1 - u) * (1 - v)])
            wts.append(w[idx[0]] * w[idx[1]] * w[idx[2]] * (1 - u) ** 2 * (1 - v))
    return np.array(pts), np.array(wts)


def frame_locals(kind):
    """Local nodes spanning the affine map: X0 and the ends of J's columns."""
    return {QUAD: [0, 2, 6], HEX: [0, 2, 6, 18], TRI: [0, 1, 2], TET: [0, 1, 2, 3]}[kind]


def element_matrices(kind, X):
    """K_e, M_e of one affine cell with frame vertices X[0..d].  Entries that vanish in exact arithmetic come out of the
    quadrature as ~1e-17 of the largest; they are set to 0 (the exact entries are rationals times the geometry: no
    non-zero one is below 1e-12 of the largest)."""
    d = dim_of(kind)
    J = (np.asarray(X[1:d + 1]) - np.asarray(X[0])).T
    Ji, det = np.linalg.inv(J), abs(np.linalg.det(J))
    m = nodes_per_cell(kind)
    K, M = np.zeros((m, m)), np.zeros((m, m))
    for xi, w in zip(*reference_rule(kind)):
        N, G = basis(kind, xi)
        g = G @ Ji
        K += w * det * g @ g.T
        M += w * det * np.outer(N, N)
    for A in (K, M):
        A[np.abs(A) <= 1e-12 * np.abs(A).max()] = 0.0
    return K, M


def assemble_KM(kind, nx, ny, nz=0):
    X = coords(kind, nx, ny, nz)
    cells = dofmap(kind, nx, ny, nz)
    n = X.shape[0]
    rows, cols, kv, mv, cache = [], [], [], [], {}
    for c in cells:
        F = X[c[frame_locals(kind)]]
        key = tuple(np.round((F - F[0]).ravel() * 1e12).astype(np.int64))
        if key not in cache:
            cache[key] = element_matrices(kind, F)
        Ke, Me = cache[key]
        rows.append(np.repeat(c, len(c)))
        cols.append(np.tile(c, len(c)))
        kv.append(Ke.ravel())
        mv.append(Me.ravel())
    r, cc = np.concatenate(rows), np.concatenate(cols)
    K = sp.csr_matrix((np.concatenate(kv), (r, cc)), shape=(n, n))
    M = sp.csr_matrix((np.concatenate(mv), (r, cc)), shape=(n, n))
    for A in (K, M):
        A.sum_duplicates()
        A.sort_indices()
    return K, M


def pattern(kind, nx, ny, nz=0):
    """Sorted CSR pattern (rowptr, col) of the scalar block: pairs of nodes that share a cell."""
    cells = dofmap(kind, nx, ny, nz)
    n = n_nodes(kind, nx, ny, nz)
    r = np.concatenate([np.repeat(c, len(c)) for c in cells])
    c = np.concatenate([np.tile(c, len(c)) for c in cells])
    P = sp.csr_matrix((np.ones(r.shape[0]), (r, c)), shape=(n, n))
    P.sum_duplicates()
    P.sort_indices()
    return P.indptr.astype(np.int64), P.indices.astype(np.int32)


def eliminate(K, M, bnodes, g1, g2, k1, k2, beta, mu):
    """DPP blocks with symmetric Dirichlet elimination (constrained rows identity, constrained columns zero) and the
    lifted right-hand side [b1, b2] (zero on constrained rows) and u0 (the boundary values)."""
    n = K.shape[0]
    a, b, c = k1 / mu, beta / mu, k2 / mu
    mask = np.zeros(n, dtype=bool)
    mask[bnodes] = True
    G1, G2 = np.zeros(n), np.zeros(n)
    G1[bnodes], G2[bnodes] = g1, g2
    A11, A22, A12 = (a * K + b * M).tocsr(), (c * K + b * M).tocsr(), (-b * M).tocsr()
    r1 = -(A11 @ G1 + A12 @ G2)
    r2 = -(A12 @ G1 + A22 @ G2)
    r1[mask], r2[mask] = 0.0, 0.0
    F, I_b = sp.diags((~mask).astype(float)), sp.diags(mask.astype(float))
    A11e, A22e = (F @ A11 @ F + I_b).tocsr(), (F @ A22 @ F + I_b).tocsr()
    A12e = (F @ A12 @ F).tocsr()
    return A11e, A22e, A12e, A12e.copy(), np.concatenate([r1, r2]), np.concatenate([G1, G2])


def monolithic(A11, A22, A12, A21):
    return sp.bmat([[A11, A12], [A21, A22]], format="csr")


def ilu0(A):
    """IKJ ILU(0) restricted to the pattern of A (explicit zeros kept), natural order."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    ip, ix, LU = A.indptr, A.indices, A.data.copy()
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
    y = np.array(r, dtype=float)
    for i in range(len(y)):
        y[i] -= LU[ip[i]:diag[i]] @ y[ix[ip[i]:diag[i]]]
    for i in range(len(y) - 1, -1, -1):
        s, e = diag[i] + 1, ip[i + 1]
        y[i] = (y[i] - LU[s:e] @ y[ix[s:e]]) / LU[diag[i]]
    return y


def gmres_left(A, b, prec, rtol, atol=1e-50, restart=30, max_it=10000):
    """Left-preconditioned GMRES(restart) from a zero guess, PETSc's test: ||P^-1 r|| <= max(rtol ||P^-1 b||, atol);
    returns (x, iterations)."""
    n = b.shape[0]
    x = np.zeros(n)
    tol = max(rtol * np.linalg.norm(prec(b)), atol)
    its = 0
    while its < max_it:
        z = prec(b - A @ x)
        beta = np.linalg.norm(z)
        if beta <= tol:
            break
        V, H = np.zeros((restart + 1, n)), np.zeros((restart + 1, restart))
        cs, sn, g = np.zeros(restart), np.zeros(restart), np.zeros(restart + 1)
        V[0], g[0] = z / beta, beta
        k_done = 0
        for k in range(restart):
            w = prec(A @ V[k])
            for j in range(k + 1):
                H[j, k] = V[j] @ w
                w = w - H[j, k] * V[j]
            H[k + 1, k] = np.linalg.norm(w)
            if H[k + 1, k] != 0:
                V[k + 1] = w / H[k + 1, k]
            for j in range(k):
                t = cs[j] * H[j, k] + sn[j] * H[j + 1, k]
                H[j + 1, k] = -sn[j] * H[j, k] + cs[j] * H[j + 1, k]
                H[j, k] = t
            den = np.hypot(H[k, k], H[k + 1, k])
            cs[k], sn[k] = H[k, k] / den, H[k + 1, k] / den
            H[k, k], H[k + 1, k] = den, 0.0
            g[k + 1], g[k] = -sn[k] * g[k], cs[k] * g[k]
            its += 1
            k_done = k + 1
            if abs(g[k + 1]) <= tol or its >= max_it:
                break
        y = np.linalg.solve(np.triu(H[:k_done, :k_done]), g[:k_done])
        x = x + y @ V[:k_done]
        if abs(g[k_done]) <= tol:
            break
    return x, its


def q1d_matrices(h):
    """The 1D quadratic element matrices (stiffness, mass) of an interval of length h, nodes 0, h/2, h."""
    M = h / 30.0 * np.array([[4.0, 2.0, -1.0], [2.0, 16.0, 2.0], [-1.0, 2.0, 4.0]])
    K = 1.0 / (3.0 * h) * np.array([[7.0, -8.0, 1.0], [-8.0, 16.0, -8.0], [1.0, -8.0, 7.0]])
    return K, M
