"""SciPy restatement of the discrete adjoint of the theta scheme, on top of ``transient_reference`` (direct ``splu`` solves),
for the tests of ``perphil_amd/csrc/pph_transient_adjoint.hip``.

Forward (``transient_reference.theta_steps``): ``d_s = T^-1 (-F A_unel p_s)``, ``p_{s+1} = p_s + d_s``, ``T = Sigma M / dt +
theta A`` eliminated.  Functional ``J = sum_{s=0..N} j_s(p_s)``, ``G_s = dj_s/dp_s``.  Backward from ``q_N = F G_N``, s = N-1 .. 0::

    w_s = T^-1 q_{s+1}                       (0 on constrained dofs)
    pm  = p_s + theta d_s,  d_s = p_{s+1} - p_s
    O0 += w1^T K pm1   O1 += w2^T K pm2   O2 += (w1 - w2)^T M (pm1 - pm2)   O3 += w1^T M d1   O4 += w2^T M d2
    q_s = F G_s + q_{s+1} - F A_unel w_s     Wsum += w_s

    dJ/dk1 = -O0/mu  dJ/dk2 = -O1/mu  dJ/dbeta = -O2/mu  dJ/dmu = (k1 O0 + k2 O1 + beta O2)/mu^2
    dJ/dS1 = -O3/dt  dJ/dS2 = -O4/dt  dJ/dp_0 (free dofs) = q_0
    dJ/d(boundary value at constrained dof c) = sum_s (G_s)_c - (A_unel Wsum)_c

Every bilinear form comes with its absolute sum (``|w1|^T |K| |pm1|`` ...): what a sum of its terms can lose to rounding, per
unit of eps.  ``point_matrix`` restates the point evaluation E (rows: points, columns: nodes) by the location rule of
``point_eval_reference``; ``E.T`` is the transposed evaluation.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import transient_reference as T  # noqa: E402

EPS = T.EPS


def csr_products(K, M):
    """x -> (K x, M x, |K| |x|, |M| |x|) for stored matrices (tests/p2_matfree.Operator.parts has the same shape)."""
    aK, aM = abs(K), abs(M)
    return lambda x: (K @ x, M @ x, aK @ abs(x), aM @ abs(x))


def step_products(parts, p0, p1, theta):
    """What the five forms of a step need of (p_s, p_{s+1}), independent of w: the products K pm_f, M (pm1 - pm2), M d_f and
    their absolute counterparts, through ``parts`` (x -> K x, M x, |K| |x|, |M| |x|)."""
    n = p0.size // 2
    d = p1 - p0
    pm = p0 + theta * d
    m1, m2, d1, d2 = pm[:n], pm[n:], d[:n], d[n:]
    P1, P2, P12, D1, D2 = parts(m1), parts(m2), parts(m1 - m2), parts(d1), parts(d2)
    return dict(val=(P1[0], P2[0], P12[1], D1[1], D2[1]), mag=(P1[2], P2[2], P12[3], D1[3], D2[3]))


def forms_of(w, prod):
    """(forms [5], absolute sums [5]) of one backward step from step_products: e.g. w1^T K pm1 and |w1|^T |K| |pm1|."""
    n = w.size // 2
    w1, w2 = w[:n], w[n:]
    left = (w1, w2, w1 - w2, w1, w2)
    return (np.array([l @ v for l, v in zip(left, prod["val"])]), np.array([abs(l) @ v for l, v in zip(left, prod["mag"])]))


def step_forms(K, M, w, p0, p1, theta):
    """(forms [5], absolute sums [5]) of one backward step on stored K and M."""
    return forms_of(w, step_products(csr_products(K, M), p0, p1, theta))


def step_operator(K, M, cf: T.Coefs, storage, theta, dt, masks):
    """The eliminated step operator T (unit rows on constrained dofs), csc."""
    n = K.shape[0]
    sig = (storage[0] / dt, storage[1] / dt)
    step_cf = T.Coefs(theta * cf.k1, theta * cf.k2, theta * cf.beta, cf.mu)
    A11, A22, A12, A21, _, _ = T.shifted_blocks(K, M, step_cf, sig, masks, (np.zeros(n), np.zeros(n)))
    return sp.bmat([[A11, A12], [A21, A22]], format="csc")


def adjoint_sweep(K, M, cf: T.Coefs, storage, theta, dt, masks, states, G, solve=None):
    """The backward recursion over ``states`` ([N + 1][2n], as theta_steps returns them) for G [N + 1][2n].  ``solve``: b -> T^-1 b
    (default: splu).  Returns a dict: terms [N, 5], sums [N, 5] (absolute sums), q0, wsum, w ([N][2n], w[s])."""
    N = len(states) - 1
    con = np.concatenate(masks)
    if solve is None:
        lu = spla.splu(step_operator(K, M, cf, storage, theta, dt, masks))
        solve = lu.solve
    A = T.unel_operator(K, M, cf)
    q = np.where(con, 0.0, G[N])
    terms, sums, ws = np.zeros((N, 5)), np.zeros((N, 5)), [None] * N
    wsum = np.zeros_like(q)
    for s in range(N - 1, -1, -1):
        w = solve(q) if np.any(q != 0.0) else np.zeros_like(q)
        w[con] = 0.0
        terms[s], sums[s] = step_forms(K, M, w, states[s], states[s + 1], theta)
        q = np.where(con, 0.0, G[s] + q - A @ w)
        wsum += w
        ws[s] = w
    return dict(terms=terms, sums=sums, q0=q, wsum=wsum, w=ws)


def gradients(K, M, cf: T.Coefs, storage, dt, masks, G, sweep):
    """dict of the gradients from a sweep: k1, k2, beta, mu, S1, S2 (floats), initial (2n, 0 on constrained dofs), bc (2n, the
    boundary gradient on constrained dofs, 0 elsewhere).  The totals are summed in step order N-1 down to 0."""
    con = np.concatenate(masks)
    tot = np.zeros(5)
    for s in range(sweep["terms"].shape[0] - 1, -1, -1):
        tot += sweep["terms"][s]
    O0, O1, O2, O3, O4 = tot
    bc = np.where(con, np.sum(G, axis=0) - T.unel_operator(K, M, cf) @ sweep["wsum"], 0.0)
    return dict(k1=-O0 / cf.mu, k2=-O1 / cf.mu, beta=-O2 / cf.mu, mu=(cf.k1 * O0 + cf.k2 * O1 + cf.beta * O2) / cf.mu ** 2,
                S1=-O3 / dt, S2=-O4 / dt, initial=sweep["q0"], bc=bc)


def point_matrix(kind, degree, nx, ny, nz, pts, tol=1e-12):
    """(E [m, n] csr, outside [m]): row m holds the basis values of the cell that holds pts[m] (located as
    point_eval_reference.evaluate_fast locates it); rows of outside points are empty."""
    import point_eval_reference as P

    LD = np.longdouble
    d = P.dim_of(kind)
    nb = P.boxes(kind, nx, ny, nz)
    A, off = P._subcell_tables(kind, degree)
    p = degree * nb + 1
    pts = np.asarray(pts, dtype=np.float64)
    c, xi, outside = P.locate_fast(kind, nx, ny, nz, pts, tol)
    Q = xi.shape[0]
    if A is None:
        sub = np.zeros(Q, np.int64)
        R = xi
    else:
        h = np.concatenate([np.ones((Q, 1), LD), xi], axis=1)
        lam_all = np.einsum("srk,pk->psr", A.astype(LD), h)
        sub = np.argmax((lam_all >= 0).all(axis=2), axis=1)
        R = lam_all[np.arange(Q), sub][:, 1:]
    Nb = P.basis_all(kind, degree, R, hess=False)[0]
    lat = (degree * c)[:, None, :] + off[sub]
    node = lat[..., 0] + p[0] * lat[..., 1]
    if d == 3:
        node = node + p[0] * p[1] * lat[..., 2]
    rows = np.repeat(np.arange(Q), node.shape[1])
    vals = np.asarray(Nb, dtype=np.float64).ravel()
    keep = ~np.repeat(outside, node.shape[1])
    E = sp.csr_matrix((vals[keep], (rows[keep], node.ravel()[keep])), shape=(Q, P.n_nodes(kind, degree, nx, ny, nz)))
    return E, outside
