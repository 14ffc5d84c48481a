"""Pathlines without a GPU: the header and the binding list carry the two entry points, every Python refusal comes before
a context exists, and the NumPy restatement (tests/trace_reference.py) is pinned - against closed forms in longdouble, and
in float64 against its own longdouble run under the derived bound - so that the GPU tests can stand on it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import trace_reference as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
IDS = [f"{TR.NAMES[c[0]]}{c[1]}x{c[2]}x{c[3]}" for c in TR.CASES]


def test_entry_points_are_declared_and_bound():
    from perphil_amd import _ffi

    header = open(os.path.join(ROOT, "include", "perphil_hip.h")).read()
    for name in ("pph_trace_pathlines", "pph_trace_pathlines_device"):
        assert name in _ffi.EXPORTS and f"int {name}(" in header and hasattr(_ffi.lib, name)


def test_refusals_come_before_any_context():
    from perphil_amd import fd, postprocessing as pp
    from perphil_amd.partition import make_slab

    P = pp.Pathlines
    assert (P.STEP_LIMIT, P.EXITED, P.STAGNANT, P.OUTSIDE) == (0, 1, 2, 3)
    mesh = fd.UnitSquareMesh(3, 2, quadrilateral=True, comm=fd.COMM_SELF)
    V1, V2 = fd.FunctionSpace(mesh, "CG", 1), fd.FunctionSpace(mesh, "CG", 2)
    vel = fd.Function(fd.VectorFunctionSpace(mesh, "CG", 1))
    seeds = np.array([[0.5, 0.5], [0.25, 0.75]])
    for f in (fd.Function(V1), fd.Function(V1 * V1), fd.Function(V2)):
        with pytest.raises(ValueError, match="CG-1 vector space"):
            pp.trace_pathlines(f, seeds, 0.1, 10)
    for bad in (dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(max_steps=0),
                dict(max_steps=2.5), dict(porosity=0.0), dict(porosity=-0.3), dict(porosity=float("nan")),
                dict(record_every=-1), dict(record_every=1.5), dict(chunk=0), dict(chunk=-4), dict(min_speed=-1.0),
                dict(min_speed=float("nan"))):
        kw = dict(dt=0.1, max_steps=10)
        kw.update(bad)
        dt, ms = kw.pop("dt"), kw.pop("max_steps")
        with pytest.raises(ValueError, match=next(iter(bad))):
            pp.trace_pathlines(vel, seeds, dt, ms, **kw)
        with pytest.raises(ValueError, match=next(iter(bad))):
            pp.travel_times(fd.Function(V1), 1.0, seeds, dt, ms, **kw)
    for s in (np.zeros((4, 3)), np.zeros(3), np.zeros((2, 2, 2)), np.zeros((4, 2), dtype=complex), np.array([["a", "b"]])):
        with pytest.raises(ValueError, match="seeds"):
            pp.trace_pathlines(vel, s, 0.1, 10)
    import torch

    with pytest.raises(ValueError, match="float64"):
        pp.trace_pathlines(vel, torch.zeros(4, 2, dtype=torch.float32), 0.1, 10)
    # a degree-2 pressure is refused as its velocity is; so is anything but a scalar pressure
    with pytest.raises(NotImplementedError, match="degree-2"):
        pp.travel_times(fd.Function(V2), 1.0, seeds, 0.1, 10)
    with pytest.raises(ValueError, match="scalar"):
        pp.travel_times(vel, 1.0, seeds, 0.1, 10)
    assert mesh._ctx is None and not mesh.__dict__.get("_ctx_deg")
    # a distributed mesh (the slab of rank 0 of 2, set by hand: no process group in this test)
    cube = fd.UnitCubeMesh(2, 2, 4, hexahedral=True, comm=fd.COMM_SELF)
    velc = fd.Function(fd.VectorFunctionSpace(cube, "CG", 1))
    pc = fd.Function(fd.FunctionSpace(cube, "CG", 1))
    cube._slab = make_slab(2, 2, 4, 2, 0)
    assert cube.distributed
    with pytest.raises(NotImplementedError, match="comm=fd.COMM_SELF"):
        pp.trace_pathlines(velc, np.full((1, 3), 0.5), 0.1, 10)
    with pytest.raises(NotImplementedError, match="comm=fd.COMM_SELF"):
        pp.travel_times(pc, 1.0, np.full((1, 3), 0.5), 0.1, 10)
    assert cube._ctx is None


@pytest.mark.parametrize("case", TR.CASES, ids=IDS)
def test_restatement_constant_field_is_straight_lines(case):
    """v constant: straight lines, exit time min_e d_e / |v_e|, the side by the tie rule, to a few longdouble roundings
    per step."""
    kind, nx, ny, nz = case
    d = TR.dim_of(kind)
    v = np.array([0.5, -0.25, 0.125])[:d]                       # (exact in binary: the nodal field is exactly constant)
    U = np.broadcast_to(v, (TR.n_nodes(kind, nx, ny, nz), d))
    X0 = np.random.default_rng(3).random((200, d))
    X0[0] = TR.TIE_SEED[:d]                                     # a tie on the first step: x wins
    dt = 1.0 / 16
    r = TR.trace(kind, nx, ny, nz, U, X0, 1.0, dt, 1000, dtype=LD)
    dist = np.where(v > 0, 1 - X0, X0).astype(LD)
    th = dist / np.abs(v).astype(LD)
    e = np.argmin(th, axis=1)
    T = th.min(axis=1)
    assert (r["status"] == TR.EXITED).all()
    assert (r["side"] == 2 * e + np.where(v[e] > 0, 2, 1)).all() and r["side"][0] == 2
    tol = LD(2.0) ** -64 * 8 * (r["steps"] + 1)
    assert (np.abs(r["time"] - T) <= tol * 2).all()
    assert (np.abs(r["end"] - (X0.astype(LD) + T[:, None] * v.astype(LD))).max(axis=1) <= tol).all()
    assert (np.abs(r["length"] - T * np.sqrt((v.astype(LD) ** 2).sum())) <= tol * 2).all()
    # floor(T / dt) full steps, then the exit step
    q = (T / LD(dt)).astype(np.float64)
    assert (np.abs(q - np.rint(q)) > 1e-9).all()
    assert (r["steps"] == np.floor(q).astype(int) + 1).all()
    assert r["steps"][0] == 1 and r["time"][0] == 2.0 ** -6 and np.array_equal(r["end"][0], [1.0, 0.0, 0.5 + 2.0 ** -9][:d])


def _affine_case(kind, nx, ny, nz, which):
    d = TR.dim_of(kind)
    c = np.full(d, 0.5)
    rng = np.random.default_rng(11 + kind)
    if which == "rotation":
        A = TR.rotation(d, 1.0)
        ang, rad = rng.random(64) * 2 * np.pi, 0.05 + 0.35 * rng.random(64)           # radius <= 0.4: never leaves
        X0 = np.full((64, d), 0.5)
        X0[:, 0] += rad * np.cos(ang)
        X0[:, 1] += rad * np.sin(ang)
        if d == 3:
            X0[:, 2] = rng.random(64)
        return A, c, X0, 0.05, 60
    A = TR.saddle(d)
    X0 = 0.5 + 0.3 * (rng.random((64, d)) - 0.5)
    return A, c, X0, 0.05, 60


@pytest.mark.parametrize("which", ("rotation", "saddle"))
@pytest.mark.parametrize("case", TR.CASES, ids=IDS)
def test_restatement_affine_field_is_the_rk4_matrix_power(case, which):
    """v = A (x - c) lies in P1 and Q1: after N full steps x_N - c = R(dt A)^N (x_0 - c), R the RK4 stability polynomial.
    Nodal values and run in longdouble; the tolerance is path_bound at longdouble's unit roundoff (the nodal values' own
    4 roundings included).  Pins all four stages and every cell crossing without reference to the kernel."""
    kind, nx, ny, nz = case
    A, c, X0, dt, N = _affine_case(kind, nx, ny, nz, which)
    U = TR.affine_field(kind, nx, ny, nz, A, c, dtype=LD)
    R = TR.rk4_matrix(LD(dt) * A.astype(LD))
    full = TR.trace(kind, nx, ny, nz, U, X0, 1.0, dt, N, dtype=LD)
    if which == "rotation":
        assert (full["status"] == TR.STEP_LIMIT).all() and (full["steps"] == N).all()
    else:
        assert (full["status"] == TR.EXITED).sum() >= 32
    checked = 0
    for n in (1, 7, N):
        r = TR.trace(kind, nx, ny, nz, U, X0, 1.0, dt, n, dtype=LD)
        sel = (r["status"] == TR.STEP_LIMIT) & (r["steps"] == n)          # n FULL steps (a saddle particle: until its exit)
        want = (X0.astype(LD) - c) @ np.linalg.matrix_power(R, n).T + c
        bound = TR.path_bound(kind, nx, ny, nz, U.astype(np.float64), 1.0, dt, r, unit=2.0 ** -64, extra_roundings=4)[0]
        err = np.abs(r["end"] - want).max(axis=1).astype(np.float64)
        assert (err[sel] <= bound[sel]).all(), (err[sel] / bound[sel]).max()
        checked += int(sel.sum())
    assert checked >= 64


@pytest.mark.parametrize("which", (0, 1), ids=("exit", "limit-stagnant"))
@pytest.mark.parametrize("case", TR.CASES, ids=IDS)
def test_float64_run_stays_within_the_bound_of_the_longdouble_run(case, which):
    kind, nx, ny, nz = case
    cfg = TR.configs(kind)[which]
    dt, max_steps, min_speed = cfg
    U = TR.smooth_field(kind, nx, ny, nz)
    S = TR.fixed_seeds(kind, nx, ny, nz)
    assert TR.lipschitz(kind, nx, ny, nz, U, 1.0) * max_steps * dt <= 5.0
    ref = TR.trace(kind, nx, ny, nz, U, S, 1.0, dt, max_steps, min_speed, dtype=LD)
    got = TR.trace(kind, nx, ny, nz, U, S, 1.0, dt, max_steps, min_speed, dtype=np.float64)
    keep = ref["margin"] >= TR.MARGIN
    assert (~keep).mean() <= 0.02, f"{(~keep).sum()} particles within {TR.MARGIN} of a decision"
    for key in ("status", "side", "steps"):
        assert (got[key][keep] == ref[key][keep]).all(), key
    if min_speed == 0.0:
        assert (ref["status"] == TR.EXITED).sum() > 900 and (ref["status"] == TR.OUTSIDE).sum() == 2
    else:
        assert min((ref["status"] == s).sum() for s in (TR.STEP_LIMIT, TR.EXITED, TR.STAGNANT)) >= 20
    b_end, b_time, b_len = TR.path_bound(kind, nx, ny, nz, U, 1.0, dt, ref)
    sel = keep & (ref["status"] != TR.OUTSIDE)
    e_end = np.abs((got["end"] - ref["end"]).astype(np.float64)).max(axis=1)
    e_time = np.abs((got["time"] - ref["time"]).astype(np.float64))
    e_len = np.abs((got["length"] - ref["length"]).astype(np.float64))
    worst = [TR.worst_ratio(e[sel], b[sel]) for e, b in ((e_end, b_end), (e_time, b_time), (e_len, b_len))]
    print(f"{TR.NAMES[kind]} {cfg}: worst error / bound: end {worst[0]:.3g} time {worst[1]:.3g} length {worst[2]:.3g}; "
          f"left out {(~keep).sum()}")
    assert max(worst) <= 1.0
    out = ref["status"] == TR.OUTSIDE
    assert np.isnan(got["end"][out]).all() and np.isnan(got["time"][out]).all() and (got["steps"][out] == 0).all()


def test_restatement_path_record_is_the_truncated_trace():
    kind, nx, ny, nz = TR.CASES[2]
    U = TR.smooth_field(kind, nx, ny, nz)
    S = TR.fixed_seeds(kind, nx, ny, nz)[::8]
    r = TR.trace(kind, nx, ny, nz, U, S, 1.0, 0.02, 40, record_every=10, dtype=np.float64)
    assert r["paths"].shape == (len(S), 5, 3)
    inside = r["status"] != TR.OUTSIDE
    assert np.array_equal(r["paths"][inside, 0], S[inside])
    for j in (1, 3):
        t = TR.trace(kind, nx, ny, nz, U, S, 1.0, 0.02, 10 * j, dtype=np.float64)
        reached = inside & (r["steps"] >= 10 * j)
        assert np.array_equal(r["paths"][reached, j], t["end"][reached])
        assert np.isnan(r["paths"][~reached, j]).all()
