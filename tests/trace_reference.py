"""NumPy restatement of pathline tracing (postprocessing.trace_pathlines / pph_trace_pathlines), written from the step rule
documented in include/perphil_hip.h, with its own location and basis code for the four cell kinds; parametrised by dtype
(np.float64 or np.longdouble).  No tests in here.

Field: v(x) = scale * u_h(x), u_h the CG-1 vector field with nodal values U[node, c] on the uniform lattice
(node = ix + (nx + 1) (iy + (ny + 1) iz)).  Location per direction: t = x n, box c = clamp(floor(t), 0, n - 1), xi = t - c.
Bases: Q1 tensor products; triangles: lower sub-cell {0, 1, 2} where xi_x + xi_y <= 1, else {1, 3, 2}; Kuhn tetrahedra:
the path 0 -> 7 along the axes in the descending order of xi.  u_h is continuous, so which of two cells a face point is
given to changes roundings only.

`trace` also returns, per particle, `margin`: the smallest distance of its trajectory to a DECISION - a stage coordinate
to 0 or 1, |k1| to min_speed, the two smallest theta of an exit step to each other, theta to dt.  A float64 run and a
longdouble run agree on every decision of a particle whose longdouble margin exceeds the path error by far; the tests leave
out particles with margin < 1e-9.

`path_bound` bounds the deviation of a float64 run (this restatement's, or the kernel's: any summation order, fused
multiply-adds allowed) from the longdouble run; its derivation stands at the function."""
from __future__ import annotations

import numpy as np

LD = np.longdouble
QUAD, TRI, HEX, TET = 0, 1, 2, 3
STEP_LIMIT, EXITED, STAGNANT, OUTSIDE = 0, 1, 2, 3
U53 = 2.0 ** -53
MARGIN = 1e-9
CASES = [(QUAD, 5, 3, 0), (TRI, 4, 5, 0), (HEX, 3, 4, 2), (TET, 3, 2, 4)]
NAMES = ("quad", "tri", "hex", "tet")


def dim_of(kind):
    return 2 if kind in (QUAD, TRI) else 3


def boxes(kind, nx, ny, nz=0):
    return np.array([nx, ny, nz][: dim_of(kind)], dtype=np.int64)


def n_nodes(kind, nx, ny, nz=0):
    return int(np.prod(boxes(kind, nx, ny, nz) + 1))


def node_coords(kind, nx, ny, nz=0, dtype=np.float64):
    """[n, d] lattice coordinates index / n in `dtype`, in node order."""
    n = boxes(kind, nx, ny, nz)
    ids = np.arange(n_nodes(kind, nx, ny, nz))
    p = n + 1
    cols = [ids % p[0], (ids // p[0]) % p[1]]
    if len(n) == 3:
        cols.append(ids // (p[0] * p[1]))
    return np.stack(cols, axis=1).astype(dtype) / n.astype(dtype)


def velocity(kind, nx, ny, nz, Ud, X, scale):
    """scale * u_h at the points X [P, d] (dtype of X; Ud [n, d] in the same dtype).  Points may lie outside the unit box:
    the clamped box's basis is then extrapolated (never used by `trace`: a stage point outside ends the stages)."""
    dt = X.dtype.type
    d = dim_of(kind)
    n = boxes(kind, nx, ny, nz)
    nd = n.astype(X.dtype)
    t = X * nd
    c = np.clip(np.floor(np.where(np.isnan(t), dt(0), t)), dt(0), nd - 1)
    xi = t - c
    ci = c.astype(np.int64)
    stride = np.array([1, n[0] + 1, (n[0] + 1) * (n[1] + 1)][:d], dtype=np.int64)
    base = (ci * stride).sum(axis=1)
    P = X.shape[0]

    def corner(bits):     # node ids of the box corner given per point as [P, d] 0/1
        return base + (bits * stride).sum(axis=1)

    v = np.zeros((P, d), X.dtype)
    if kind in (QUAD, HEX):
        for b in range(1 << d):
            bits = np.array([(b >> e) & 1 for e in range(d)])
            N = np.ones(P, X.dtype)
            for e in range(d):
                N = N * (xi[:, e] if bits[e] else 1 - xi[:, e])
            v = v + N[:, None] * Ud[corner(np.broadcast_to(bits, (P, d)))]
    elif kind == TRI:
        lower = xi[:, 0] + xi[:, 1] <= 1
        lam_lo = [1 - xi[:, 0] - xi[:, 1], xi[:, 0], xi[:, 1]]
        lam_up = [1 - xi[:, 1], xi[:, 0] + xi[:, 1] - 1, 1 - xi[:, 0]]
        for r in range(3):
            cb = np.where(lower, (0, 1, 2)[r], (1, 3, 2)[r])
            bits = np.stack([cb & 1, (cb >> 1) & 1], axis=1)
            v = v + np.where(lower, lam_lo[r], lam_up[r])[:, None] * Ud[corner(bits)]
    else:
        order = np.argsort(-xi, axis=1, kind="stable")             # axes in descending order of xi
        xs = np.take_along_axis(xi, order, axis=1)
        lam = [1 - xs[:, 0], xs[:, 0] - xs[:, 1], xs[:, 1] - xs[:, 2], xs[:, 2]]
        bits = np.zeros((P, 3), np.int64)
        v = v + lam[0][:, None] * Ud[corner(bits)]
        for r in range(3):
            bits = bits.copy()
            bits[np.arange(P), order[:, r]] = 1
            v = v + lam[r + 1][:, None] * Ud[corner(bits)]
    return v * dt(scale)


def _inside(Y):
    return np.all((Y >= 0) & (Y <= 1), axis=1)


def _norm(V):
    q = V[:, 0] * V[:, 0]
    for e in range(1, V.shape[1]):
        q = q + V[:, e] * V[:, e]
    return np.sqrt(q)


def _wall(Y):
    """Per point: smallest distance of a coordinate to 0 or 1 (NaN -> 0)."""
    w = np.minimum(np.abs(Y), np.abs(1 - Y)).min(axis=1).astype(np.float64)
    return np.where(np.isnan(w), 0.0, w)


def trace(kind, nx, ny, nz, U, seeds, scale, dt, max_steps, min_speed=0.0, record_every=0, dtype=LD):
    """The step rule, vectorised over the particles.  Returns a dict: end [m, d], time, length (dtype), steps, status, side
    (int), margin (float64), exit_speed (|k1_e| of the exit direction, float64; NaN unless exited), paths [m, n_rec, d] or
    None."""
    T = np.dtype(dtype).type
    d = dim_of(kind)
    Ud = np.asarray(U).reshape(-1, d).astype(dtype)      # (float64 nodal values, or longdouble ones for the closed forms)
    X = np.asarray(seeds, dtype=np.float64).reshape(-1, d).astype(dtype)
    m = X.shape[0]
    dtt, hdt, dt6, ms = T(dt), T(0.5) * T(dt), T(dt) / T(6), T(min_speed)
    t = np.zeros(m, dtype); s = np.zeros(m, dtype); k = np.zeros(m, np.int64)
    status = np.full(m, -1, np.int64); side = np.zeros(m, np.int64)
    margin = np.full(m, np.inf); exit_speed = np.full(m, np.nan)
    out = ~_inside(X) if m else np.zeros(0, bool)
    status[out] = OUTSIDE
    n_rec = max_steps // record_every + 1 if record_every > 0 else 0
    paths = np.full((m, n_rec, d), np.nan, dtype) if n_rec else None
    if n_rec:
        paths[~out, 0] = X[~out]
    X[out] = np.nan; t[out] = np.nan; s[out] = np.nan
    while True:
        act = np.nonzero(status < 0)[0]
        if act.size == 0:
            break
        x = X[act]
        k1 = velocity(kind, nx, ny, nz, Ud, x, scale)
        sp = _norm(k1)
        mg = np.abs((sp - ms).astype(np.float64))
        stag = sp <= ms
        ok = ~stag
        y = x + hdt * k1
        mg = np.minimum(mg, np.where(ok, _wall(y), np.inf)); ok = ok & _inside(y)
        kk = velocity(kind, nx, ny, nz, Ud, np.where(ok[:, None], y, x), scale)
        acc = k1 + 2 * kk
        y = x + hdt * kk
        mg = np.minimum(mg, np.where(ok, _wall(y), np.inf)); ok = ok & _inside(y)
        kk = velocity(kind, nx, ny, nz, Ud, np.where(ok[:, None], y, x), scale)
        acc = acc + 2 * kk
        y = x + dtt * kk
        mg = np.minimum(mg, np.where(ok, _wall(y), np.inf)); ok = ok & _inside(y)
        kk = velocity(kind, nx, ny, nz, Ud, np.where(ok[:, None], y, x), scale)
        acc = acc + kk
        y = x + dt6 * acc
        mg = np.minimum(mg, np.where(ok, _wall(y), np.inf)); ok = ok & _inside(y)
        # exit step for the rest (not stagnant, some stage point outside)
        ex = ~stag & ~ok
        with np.errstate(divide="ignore", invalid="ignore"):
            th = np.where(k1 != 0, np.where(k1 > 0, 1 - x, x) / np.abs(k1), T(np.inf))
        th = np.where(np.isnan(th), T(np.inf), th)
        emin = np.argmin(th, axis=1)                                   # (first minimum: the lowest direction wins a tie)
        theta = th[np.arange(act.size), emin]
        ths = np.sort(th.astype(np.float64), axis=1)
        mg = np.minimum(mg, np.where(ex, np.minimum(ths[:, 1] - ths[:, 0], np.abs(ths[:, 0] - float(dt))), np.inf))
        leave = ex & (theta <= dtt)
        euler = ex & ~leave
        xn = x.copy(); tn = t[act].copy(); sn = s[act].copy()
        xn[ok] = y[ok]; tn[ok] += dtt; sn[ok] += _norm(y[ok] - x[ok])
        if leave.any():
            i = np.nonzero(leave)[0]
            xe = x[i] + theta[i, None] * k1[i]
            pos = k1[i, emin[i]] > 0
            xe[np.arange(i.size), emin[i]] = np.where(pos, T(1), T(0))
            xn[i] = xe; tn[i] += theta[i]; sn[i] += theta[i] * sp[i]
            side[act[i]] = 2 * emin[i] + np.where(pos, 2, 1)
            exit_speed[act[i]] = np.abs(k1[i, emin[i]]).astype(np.float64)
        if euler.any():
            i = np.nonzero(euler)[0]
            xe = np.clip(x[i] + dtt * k1[i], T(0), T(1))
            xn[i] = xe; tn[i] += dtt; sn[i] += _norm(xe - x[i])
        moved = ~stag
        X[act] = xn; t[act] = tn; s[act] = sn
        k[act[moved]] += 1
        margin[act] = np.minimum(margin[act], mg)
        if n_rec:
            r = act[moved & (k[act] % record_every == 0)]
            paths[r, k[r] // record_every] = X[r]
        status[act[stag]] = STAGNANT
        status[act[leave]] = EXITED
        lim = act[moved & ~leave & (k[act] >= max_steps)]
        status[lim] = STEP_LIMIT
    return dict(end=X, time=t, length=s, steps=k, status=status, side=side, margin=margin, exit_speed=exit_speed, paths=paths)


# ---------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------
def lipschitz(kind, nx, ny, nz, U, scale):
    """L with |v(x) - v(y)|_inf <= L |x - y|_inf: along direction e the derivative of a CG-1 component is, on all four cell
    kinds, a convex combination of (nodal difference along an e-edge) n_e, so L = |scale| sum_e n_e D_e with D_e the
    largest nodal difference (any component) along an edge in direction e."""
    d = dim_of(kind)
    n = boxes(kind, nx, ny, nz)
    A = np.asarray(U, dtype=np.float64).reshape(*(n[::-1] + 1), d)      # [.., iy, ix, c]
    L = 0.0
    for e in range(d):
        L += n[e] * np.abs(np.diff(A, axis=d - 1 - e)).max()
    return abs(scale) * L


def gamma_velocity(kind):
    """Roundings on the longest path from xi to a velocity component, without fused multiply-adds: Q1: 1 - xi (1), the
    product of d weights (d - 1), times u (1), the sum of 2^d terms (2^d - 1); P1: a barycentric coordinate (<= 2), times u
    (1), the sum of d + 1 terms (d); then the scale (1), and 1 for second-order terms and the longdouble run's own rounding."""
    d = dim_of(kind)
    return (d + 2 ** d if kind in (QUAD, HEX) else 3 + d) + 2


def path_bound(kind, nx, ny, nz, U, scale, dt, ref, unit=U53, extra_roundings=0):
    """Per particle: bounds (end, time, length) on |float64 run - longdouble run| in the maximum norm, for particles
    whose decisions agree.  `ref`: the longdouble `trace`.

    One evaluation of v at a given point, in float64: the rounding of t = x n moves the point by at most 2^-53 per
    coordinate (|x| <= 1), which L carries into v; the basis and the sum add gamma roundings relative to sum |N_b| |u_b|
    <= vmax = |scale| max |U| (the basis is non-negative and sums to 1 inside).  A device may contract a multiply and an
    add: that changes which roundings occur, not their size - allowed for by a factor 2 on every operation count.
        a = 2^-53 (2 gamma vmax + L)
    One step.  A stage point x + h k carries the error of k times h, plus two roundings (<= 2 * 2 * 2^-53: coordinates
    and increments are at most 1 in size):  p = 4 * 2^-53;  e1 = a, e2 = a + L (dt/2 e1 + p), e3 = a + L (dt/2 e2 + p),
    e4 = a + L (dt e3 + p).  The combination k1 + 2 k2 + 2 k3 + k4 (3 additions of at most 6 vmax), dt / 6 (1) and its product
    (1), the final addition (1, result at most 1):
        rho = dt/6 (e1 + 2 e2 + 2 e3 + e4) + 2 * 2^-53 (5 dt vmax + 1)
    The exact step map is Lipschitz with 1 + dt L + .. + (dt L)^4 / 24 <= exp(dt L) (an Euler fall-back step with 1 + dt L, the
    clamp with 1), so after k steps   E_k <= k rho exp(L k dt).
    Time: k additions of dt to at most k dt: 2 k 2^-53 k dt.  Length: per step |xn - x| changes by at most 2 E_k, and its own
    arithmetic (d squares and additions, a root, the addition to s) by 2 (d + 3) 2^-53 times the step length (<= dt vmax
    sqrt(d)) plus 2^-53 s.
    Exit step: theta = d_e / |k1_e| with d_e off by E_k + 2^-53 and k1_e by e1: dtheta = (E_k + 2^-53 + theta e1) / |k1_e| +
    4 * 2^-53 theta; the end point moves by E_k + dtheta vmax + theta e1 + 4 * 2^-53, the time by dtheta, the length by
    sqrt(d) (dtheta vmax + theta e1) + 4 * 2^-53 theta vmax.
    `unit`: the unit roundoff (2^-64 bounds a longdouble run against exact arithmetic); `extra_roundings`: roundings the
    nodal values themselves carry relative to the field a closed form describes (added to gamma)."""
    d = dim_of(kind)
    u = unit
    vmax = abs(scale) * float(np.abs(np.asarray(U, dtype=np.float64)).max())
    L = lipschitz(kind, nx, ny, nz, U, scale)
    a = u * ((2 * gamma_velocity(kind) + extra_roundings) * vmax + L)
    p = 4 * u
    e1 = a
    e2 = a + L * (dt / 2 * e1 + p)
    e3 = a + L * (dt / 2 * e2 + p)
    e4 = a + L * (dt * e3 + p)
    rho = dt / 6 * (e1 + 2 * e2 + 2 * e3 + e4) + 2 * u * (5 * dt * vmax + 1)
    k = np.asarray(ref["steps"], dtype=np.float64)
    E = k * rho * np.exp(L * k * dt)
    b_time = 2 * k * u * k * dt
    s = np.nan_to_num(np.asarray(ref["length"], dtype=np.float64))
    b_len = k * (2 * E + 2 * (d + 3) * u * dt * vmax * np.sqrt(d)) + k * u * (s + k * dt * vmax)
    exited = np.asarray(ref["status"]) == EXITED
    theta = dt                                                          # (theta <= dt)
    ke = np.where(exited, ref["exit_speed"], 1.0)
    dth = np.where(exited, (E + u + theta * e1) / ke + 4 * u * theta, 0.0)
    b_end = E + np.where(exited, dth * vmax + theta * e1 + 4 * u, 0.0)
    b_time = b_time + dth
    b_len = b_len + np.where(exited, np.sqrt(d) * (dth * vmax + theta * e1) + 4 * u * theta * vmax, 0.0)
    return b_end, b_time, b_len


def worst_ratio(err, bound):
    """max err / bound; a zero bound (a particle that took no step) allows no error at all: inf if there is one."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(q))


# ---------------------------------------------------------------------------------------------------------------
# the inputs the host and GPU tests share
# ---------------------------------------------------------------------------------------------------------------
N_RANDOM = 1000


def smooth_field(kind, nx, ny, nz=0, seed=0):
    """A low-order polynomial field interpolated at the nodes plus a small random perturbation (1e-3): smooth enough that
    L max_steps dt <= 5 at the steps the tests take, rough enough that no two cells carry the same gradient."""
    d = dim_of(kind)
    rng = np.random.default_rng(100 + 10 * kind + seed)
    X = node_coords(kind, nx, ny, nz)
    x, y = X[:, 0], X[:, 1]
    z = X[:, 2] if d == 3 else 0 * x
    cols = [0.6 + 0.3 * y - 0.2 * x * x + 0.1 * z, 0.25 - 0.5 * x * y + 0.2 * z * z, 0.15 + 0.3 * x - 0.35 * y * z][:d]
    return np.stack(cols, axis=1) + 1e-3 * rng.standard_normal((X.shape[0], d))


def configs(kind):
    """(dt, max_steps, min_speed) of the two runs on smooth_field: nearly every particle exits / the step limit and the
    speed threshold (inside the field's range of speeds: 0.48 .. 0.93 in 2D, 0.66 .. 1.08 in 3D) both bite."""
    return [(0.02, 100, 0.0), (0.02, 25, 0.6 if dim_of(kind) == 2 else 0.72)]


def deliberate_seeds(kind, nx, ny, nz=0):
    """On nodes, on faces between boxes, on the domain boundary, two corners, one point outside, one NaN."""
    d = dim_of(kind)
    n = boxes(kind, nx, ny, nz)
    rng = np.random.default_rng(77 + kind)
    out = []
    for _ in range(6):                                   # interior nodes
        out.append(np.array([rng.integers(1, max(2, n[e])) / n[e] for e in range(d)]))
    for e in range(d):                                   # faces between boxes (one coordinate on a lattice plane)
        for _ in range(3):
            y = rng.random(d)
            y[e] = rng.integers(1, max(2, n[e])) / n[e]
            out.append(y)
    for e in range(d):                                   # the domain boundary
        for v in (0.0, 1.0):
            y = rng.random(d)
            y[e] = v
            out.append(y)
    out.append(np.zeros(d))
    out.append(np.ones(d))
    y = rng.random(d); y[0] = 1.0 + 1e-3
    out.append(y)                                        # outside
    y = rng.random(d); y[d - 1] = np.nan
    out.append(y)                                        # NaN
    return np.array(out)


def fixed_seeds(kind, nx, ny, nz=0):
    rnd = np.random.default_rng(500 + kind).random((N_RANDOM, dim_of(kind)))
    return np.concatenate([rnd, deliberate_seeds(kind, nx, ny, nz)], axis=0)


# in the constant field (0.5, -0.25, 0.125) with dt = 1/16: the stage point x + dt/2 k1 is outside on the first step, and the
# faces x = 1 and y = 0 are both exactly 2^-6 time units away (every number involved is a short dyadic rational)
TIE_SEED = np.array([1 - 2.0 ** -7, 2.0 ** -8, 0.5])


def rk4_matrix(Z):
    """R(Z) = I + Z + Z^2 / 2 + Z^3 / 6 + Z^4 / 24 (longdouble)."""
    Z = np.asarray(Z, dtype=LD)
    I = np.eye(Z.shape[0], dtype=LD)
    Z2 = Z @ Z
    return I + Z + Z2 / 2 + Z2 @ Z / 6 + Z2 @ Z2 / 24


def affine_field(kind, nx, ny, nz, A, c, dtype=np.float64):
    """Nodal values of v = A (x - c) (lies in P1 and in Q1)."""
    X = node_coords(kind, nx, ny, nz, dtype)
    return (X - np.asarray(c, dtype=dtype)[None, :]) @ np.asarray(A, dtype=dtype).T


def rotation(d, omega=1.0):
    A = np.zeros((d, d))
    A[0, 1], A[1, 0] = -omega, omega
    return A


def saddle(d):
    return np.diag([1.0, -1.0, -0.5][:d])
