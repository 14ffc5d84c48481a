"""NumPy / SciPy restatement of transient DPP runs with sources, on top of ``transient_reference``,
``transient_adjoint_reference`` and ``oracle.dpp_oracle``, for the tests of ``perphil_amd/csrc/pph_sources.hip``.

Model, with load vectors L_k (2n, field-major, constant in time) and rates r_k(t), q > 0 injecting::

    S1 dp1/dt - div(k1/mu grad p1) + beta/mu (p1 - p2) = q1(x, t)
    S2 dp2/dt - div(k2/mu grad p2) - beta/mu (p1 - p2) = q2(x, t)
    (Sigma M / dt + theta A) d = F (-A_unel p^s + sum_k c[s][k] L_k),   c[s][k] = theta r_k(t_{s+1}) + (1 - theta) r_k(t_s)

Loads.  A well at x in network f: ``L[f n + node] = phi_node(x)`` on the nodes of a cell that holds x - degree 1: the oracle's
own shape functions on the oracle's dof map (``oracle_point_load``; CG basis functions are continuous, so which of the cells
that share a face holds the point does not change the load); degree 2: ``transient_adjoint_reference.point_matrix``.  A
distributed source f: the consistent load ``M f`` in its network.

Rate gradients.  The sources depend neither on the state nor on the parameters: the backward recursion of
``transient_adjoint_reference.adjoint_sweep`` is unchanged, and ``dJ/dc[s][k] = G[s][k] = w_s^T F L_k``;
``dJ/dr_k(t_j) = theta G[j-1][k] + (1 - theta) G[j][k]`` with rows outside 0 .. N-1 taken as 0.

Closed form (Q1 cells, homogeneous Dirichlet data on the whole boundary): the sine mode phi is an eigenvector of K and M
(``transient_reference.mode_eigenvalues``), so a distributed source ``f = phi`` in network f has the load ``lam_M phi e_f`` and
the amplitudes of ``(c1, c2) phi`` follow ``c_{s+1} = G c_s + (S lam_M / dt + theta Ah)^-1 lam_M c[s] e_f``.
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

import transient_adjoint_reference as A  # noqa: E402
import transient_reference as T  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

EPS = T.EPS
LOCATE_TOL = 1e-12


def coefficients(rates, theta: float) -> np.ndarray:
    """c[s][k] from the rates [N + 1][K] at t_0 .. t_N."""
    R = np.asarray(rates, dtype=np.float64)
    return theta * R[1:] + (1.0 - theta) * R[:-1]


def oracle_point_load(om, x) -> np.ndarray:
    """[n] phi_node(x) on the oracle's degree-1 mesh ``om``: its shape functions (corner-bit multilinear functions on boxes,
    barycentric coordinates on simplices) on the cell that holds x best (largest smallest coordinate: a point within the
    tolerance of a face is evaluated where it lies, not clamped onto the face); zeros for a point outside.  A point within the
    tolerance outside the DOMAIN is clamped onto it, as the point evaluation clamps it."""
    x = np.asarray(x, dtype=np.float64)
    X = om.coords[om.cells]                                   # [nc, m, d]
    L = np.zeros(om.num_nodes)
    if om.kind in (o.CELL_QUAD, o.CELL_HEX):
        x0, h = X[:, 0, :], X[:, -1, :] - X[:, 0, :]
        xi = (x[None] - x0) / h
        inside = np.all((xi >= -LOCATE_TOL) & (xi <= 1.0 + LOCATE_TOL), axis=1)
        if not inside.any():
            return L
        xi = (np.clip(x, 0.0, 1.0)[None] - x0) / h
        c = int(np.argmax(np.minimum(xi, 1.0 - xi).min(axis=1)))
        t = np.clip(xi[c], 0.0, 1.0)
        for a in range(X.shape[1]):
            L[om.cells[c, a]] += np.prod([t[e] if (a >> e) & 1 else 1.0 - t[e] for e in range(om.dim)])
        return L
    E = X[:, 1:, :] - X[:, :1, :]                             # edge vectors as rows
    Einv = np.linalg.inv(E)

    def barycentric(y):
        lam = np.einsum("cd,cde->ce", y[None] - X[:, 0, :], Einv)
        return np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1)

    if not np.all(barycentric(x) >= -LOCATE_TOL, axis=1).any():
        return L
    lam = barycentric(np.clip(x, 0.0, 1.0))
    c = int(np.argmax(lam.min(axis=1)))
    for a in range(X.shape[1]):
        L[om.cells[c, a]] += lam[c, a]
    return L


def point_loads(kind, degree, nx, ny, nz, pts, fields, om=None):
    """(L [m][2n], outside [m]) of wells at pts [m, dim] in the networks fields [m]."""
    pts = np.asarray(pts, dtype=np.float64)
    if degree == 1:
        om = om or o.build_mesh(2 if kind in (o.CELL_QUAD, o.CELL_TRI) else 3, kind, nx, ny, nz)
        rows = np.stack([oracle_point_load(om, x) for x in pts]) if len(pts) else np.zeros((0, om.num_nodes))
        outside = ~(np.abs(rows).sum(axis=1) > 0.0)
    else:
        E, outside = A.point_matrix(kind, degree, nx, ny, nz, pts, LOCATE_TOL)
        rows = E.toarray()
    n = rows.shape[1]
    L = np.zeros((len(pts), 2 * n))
    for p, f in enumerate(fields):
        L[p, f * n:(f + 1) * n] = rows[p]
    return L, outside


def mass_load(M, f, network: int) -> np.ndarray:
    """(M f in the given network, 0 in the other)."""
    n = M.shape[0]
    L = np.zeros(2 * n)
    L[network * n:(network + 1) * n] = M @ np.asarray(f, dtype=np.float64)
    return L


def apply_loads(b, loads, c, masks):
    """(b + F sum_k c[k] L_k, sum_k |c[k]| |L_k|): the result and what the sum can lose to rounding, per unit of eps."""
    loads = np.asarray(loads, dtype=np.float64)
    add = np.asarray(c, dtype=np.float64) @ loads
    mag = np.abs(np.asarray(c, dtype=np.float64)) @ np.abs(loads)
    con = np.concatenate(masks)
    return np.where(con, b, b + add), mag


def theta_steps(K, M, cf: T.Coefs, storage, theta: float, dt: float, masks, g, p0, nsteps: int, loads, coef):
    """``transient_reference.theta_steps`` with the load term: b_s = F (-A_unel p_s + sum_k coef[s][k] L_k).  Returns
    (states [nsteps + 1][2n], rhs norms, increment norms)."""
    con = np.concatenate(masks)
    lu = spla.splu(A.step_operator(K, M, cf, storage, theta, dt, masks))
    loads = np.asarray(loads, dtype=np.float64)
    p = np.where(con, np.concatenate(g), np.asarray(p0, dtype=np.float64))
    states, bn, dn = [p.copy()], [], []
    for s in range(nsteps):
        b = T.step_rhs(K, M, cf, masks, p) + np.where(con, 0.0, np.asarray(coef[s], dtype=np.float64) @ loads)
        nb = float(np.linalg.norm(b))
        d = lu.solve(b) if nb > 0.0 else np.zeros_like(b)
        d[con] = 0.0
        p = p + d
        bn.append(nb)
        dn.append(float(np.linalg.norm(d)))
        states.append(p.copy())
    return states, np.array(bn), np.array(dn)


def source_gradients(sweep, loads, masks):
    """(G [N][K], absolute sums [N][K]) with G[s][k] = w_s^T F L_k from an ``adjoint_sweep`` (exact algebra: its w come from
    splu)."""
    con = np.concatenate(masks)
    FL = np.where(con[None], 0.0, np.asarray(loads, dtype=np.float64))
    W = np.stack(sweep["w"])
    return W @ FL.T, np.abs(W) @ np.abs(FL).T


def rate_gradients(G, theta: float) -> np.ndarray:
    """dJ/dr_k(t_j) [N + 1][K] from G [N][K]."""
    N, K = G.shape
    Z = np.zeros((N + 2, K))
    Z[1:N + 1] = G
    return theta * Z[:N + 1] + (1.0 - theta) * Z[1:]


def closed_form_source_amplitudes(dim, nx, ny, nz, cf: T.Coefs, storage, theta, dt, c0, coef, network: int):
    """Amplitudes [N + 1][2] of (c1, c2) phi under the distributed source f = phi in ``network`` with coefficients coef [N]."""
    lam_k, lam_m = T.mode_eigenvalues(dim, nx, ny, nz)
    a, b, c = cf.abc
    Ah = np.array([[a * lam_k + b * lam_m, -b * lam_m], [-b * lam_m, c * lam_k + b * lam_m]])
    Sm = np.diag(np.asarray(storage, dtype=np.float64)) * lam_m / dt
    G = T.amplification(lam_k, lam_m, cf, storage, theta, dt)
    e = np.zeros(2)
    e[network] = 1.0
    out = [np.asarray(c0, dtype=np.float64)]
    for s in range(len(coef)):
        out.append(G @ out[-1] + np.linalg.solve(Sm + theta * Ah, lam_m * coef[s] * e))
    return out
