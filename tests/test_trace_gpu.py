"""Pathlines on the device (pph_trace_pathlines, postprocessing.trace_pathlines / travel_times) against the longdouble
restatement of tests/trace_reference.py, on all four cell kinds.

Integers (status, side, steps) are compared exactly and values under trace_reference.path_bound, on the particles whose
longdouble trajectory stays 1e-9 away from every decision (at most 2 % may be left out).  Every comparison prints its worst
ratio error / bound before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from perphil_amd import _ffi, fd, postprocessing as pp  # noqa: E402
import trace_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
IDS = [f"{TR.NAMES[c[0]]}{c[1]}x{c[2]}x{c[3]}" for c in TR.CASES]
P = pp.Pathlines


@functools.lru_cache(maxsize=None)
def _space(case):
    kind, nx, ny, nz = case
    mesh = fd.Mesh(TR.dim_of(kind), kind, nx, ny, nz, comm=fd.COMM_SELF)
    return fd.VectorFunctionSpace(mesh, "CG", 1)


def _velocity(case, U, device=False):
    u = np.ascontiguousarray(U, dtype=np.float64).reshape(-1).copy()
    return fd.Function(_space(case), torch.from_numpy(u).cuda() if device else u)


@functools.lru_cache(maxsize=None)
def _smooth(case):
    """The shared inputs and longdouble references on smooth_field (computed once; never modified)."""
    kind, nx, ny, nz = case
    U = TR.smooth_field(kind, nx, ny, nz)
    S = TR.fixed_seeds(kind, nx, ny, nz)
    refs = [TR.trace(kind, nx, ny, nz, U, S, 1.0, dt, ms, msp, dtype=LD) for dt, ms, msp in TR.configs(kind)]
    for a in (U, S):
        a.setflags(write=False)
    return U, S, refs


def _compare(case, U, scale, dt, got, ref, what, extra_roundings=0, want=None):
    """status / side / steps exactly and end / time / length under path_bound, on the kept particles.  `want`: closed-form
    end points compared instead of the restatement's (then with the nodal values' own roundings in the bound)."""
    kind, nx, ny, nz = case
    keep = ref["margin"] >= TR.MARGIN
    left = float((~keep).mean()) if keep.size else 0.0
    assert left <= 0.02, f"{what}: {(~keep).sum()} particles within {TR.MARGIN} of a decision"
    for key in ("status", "side", "steps"):
        assert np.array_equal(np.asarray(getattr(got, key))[keep], ref[key][keep]), f"{what}: {key}"
    b_end, b_time, b_len = TR.path_bound(kind, nx, ny, nz, U, scale, dt, ref, extra_roundings=extra_roundings)
    sel = keep & (ref["status"] != TR.OUTSIDE)
    end_ref = ref["end"] if want is None else want
    e_end = np.abs((got.end.astype(LD) - end_ref).astype(np.float64)).max(axis=1)
    e_time = np.abs((got.time.astype(LD) - ref["time"]).astype(np.float64))
    e_len = np.abs((got.length.astype(LD) - ref["length"]).astype(np.float64))
    worst = [TR.worst_ratio(e[sel], b[sel]) for e, b in ((e_end, b_end), (e_time, b_time), (e_len, b_len))]
    print(f"{what}: worst error / bound: end {worst[0]:.3g} time {worst[1]:.3g} length {worst[2]:.3g}; left out "
          f"{(~keep).sum()} of {keep.size}")
    assert max(worst) <= 1.0, what
    out = ref["status"] == TR.OUTSIDE
    assert np.isnan(got.end[out]).all() and np.isnan(got.time[out]).all() and np.isnan(got.length[out]).all()
    assert got.counts == {n: int((ref["status"] == s).sum()) for s, n in enumerate(pp._STATUS_NAMES)} or not keep.all()
    assert sum(got.counts.values()) == keep.size


@pytest.mark.parametrize("which", (0, 1), ids=("exit", "limit-stagnant"))
@pytest.mark.parametrize("case", TR.CASES, ids=IDS)
def test_random_smooth_field_against_the_restatement(case, which):
    U, S, refs = _smooth(case)
    dt, max_steps, min_speed = TR.configs(case[0])[which]
    assert TR.lipschitz(*case, U, 1.0) * max_steps * dt <= 5.0
    got = pp.trace_pathlines(_velocity(case, U), S, dt, max_steps, min_speed=min_speed)
    assert isinstance(got.end, np.ndarray) and got.end.shape == S.shape and got.paths is None
    _compare(case, U, 1.0, dt, got, refs[which], f"{TR.NAMES[case[0]]} {('exit', 'limit-stagnant')[which]}")


@pytest.mark.parametrize("case", TR.CASES, ids=IDS)
def test_porosity_and_backward_scale_the_field(case):
    """scale = -1 / porosity: the restatement with that scale (1 / 0.25 is exact, so both sides use the same number)."""
    kind, nx, ny, nz = case
    U, S, _ = _smooth(case)
    S = S[::5]
    dt, max_steps = 0.005, 100
    ref = TR.trace(kind, nx, ny, nz, U, S, -4.0, dt, max_steps, dtype=LD)
    assert TR.lipschitz(*case, U, -4.0) * max_steps * dt <= 5.0
    got = pp.trace_pathlines(_velocity(case, U), S, dt, max_steps, porosity=0.25, backward=True)
    _compare(case, U, -4.0, dt, got, ref, f"{TR.NAMES[kind]} backward")


@pytest.mark.parametrize("case", TR.CASES, ids=IDS)
def test_constant_field_closed_form(case):
    kind, nx, ny, nz = case
    d = TR.dim_of(kind)
    v = np.array([0.5, -0.25, 0.125])[:d]
    U = np.broadcast_to(v, (TR.n_nodes(kind, nx, ny, nz), d)).copy()
    X0 = np.random.default_rng(3).random((200, d))
    X0[0] = TR.TIE_SEED[:d]
    dt = 1.0 / 16
    ref = TR.trace(kind, nx, ny, nz, U, X0, 1.0, dt, 1000, dtype=LD)
    got = pp.trace_pathlines(_velocity(case, U), X0, dt, 1000)
    # the tie is decided in exact arithmetic (every number of particle 0 is a short dyadic rational, fused or not): x wins
    assert got.status[0] == P.EXITED and got.side[0] == 2 and got.steps[0] == 1 and got.time[0] == 2.0 ** -6
    assert np.array_equal(got.end[0], [1.0, 0.0, 0.5 + 2.0 ** -9][:d]) and got.length[0] == 2.0 ** -6 * np.sqrt((v * v).sum())
    T = (np.where(v > 0, 1 - X0, X0).astype(LD) / np.abs(v).astype(LD)).min(axis=1)
    _compare(case, U, 1.0, dt, got, ref, f"{TR.NAMES[kind]} constant", want=X0.astype(LD) + T[:, None] * v.astype(LD))


@pytest.mark.parametrize("which", ("rotation", "saddle"))
@pytest.mark.parametrize("case", TR.CASES, ids=IDS)
def test_affine_field_closed_form(case, which):
    """v = A (x - c): against the restatement on the same float64 nodal values, and - for the particles that took N full
    steps - against R(dt A)^N (x0 - c) + c with the nodal values' own 4 roundings added to the bound."""
    from test_trace_host import _affine_case

    kind, nx, ny, nz = case
    A, c, X0, dt, N = _affine_case(kind, nx, ny, nz, which)
    U = TR.affine_field(kind, nx, ny, nz, A, c)
    ref = TR.trace(kind, nx, ny, nz, U, X0, 1.0, dt, N, dtype=LD)
    got = pp.trace_pathlines(_velocity(case, U), X0, dt, N)
    _compare(case, U, 1.0, dt, got, ref, f"{TR.NAMES[kind]} {which}")
    full = (ref["status"] == TR.STEP_LIMIT) & (ref["margin"] >= TR.MARGIN)
    assert full.sum() >= (64 if which == "rotation" else 1)
    want = (X0.astype(LD) - c) @ np.linalg.matrix_power(TR.rk4_matrix(LD(dt) * A.astype(LD)), N).T + c
    bound = TR.path_bound(kind, nx, ny, nz, U, 1.0, dt, ref, extra_roundings=4)[0]
    err = np.abs((got.end.astype(LD) - want).astype(np.float64)).max(axis=1)
    print(f"{TR.NAMES[kind]} {which}: closed form, worst error / bound {TR.worst_ratio(err[full], bound[full]):.3g}")
    assert (err[full] <= bound[full]).all()


def _fields(r):
    return [np.asarray(a) for a in (r.end, r.time, r.length, r.steps, r.status, r.side)] + \
        ([] if r.paths is None else [np.asarray(r.paths)])


def _same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(_fields(a), _fields(b)))


@pytest.mark.parametrize("case", TR.CASES, ids=IDS)
def test_results_do_not_depend_on_the_schedule(case):
    U, S, _ = _smooth(case)
    dt, max_steps, min_speed = TR.configs(case[0])[1]
    f = _velocity(case, U)
    base = pp.trace_pathlines(f, S, dt, max_steps, min_speed=min_speed, record_every=5)
    again = pp.trace_pathlines(f, S, dt, max_steps, min_speed=min_speed, record_every=5)
    assert _same_bits(base, again) and base.counts == again.counts
    for chunk in (1, 7, max_steps):
        r = pp.trace_pathlines(f, S, dt, max_steps, min_speed=min_speed, record_every=5, chunk=chunk)
        assert _same_bits(base, r) and r.counts == base.counts, chunk


@pytest.mark.parametrize("m", (0, 1, 65))
def test_batch_sizes(m):
    """The empty batch, a single lane and a wave's tail: the first m of the fixed seeds give the first m results."""
    case = TR.CASES[2]
    U, S, _ = _smooth(case)
    dt, max_steps, min_speed = TR.configs(case[0])[1]
    f = _velocity(case, U)
    whole = pp.trace_pathlines(f, S, dt, max_steps, min_speed=min_speed, record_every=5)
    r = pp.trace_pathlines(f, S[:m], dt, max_steps, min_speed=min_speed, record_every=5, chunk=3)
    assert r.end.shape == (m, 3) and r.time.shape == (m,) and r.steps.shape == (m,) and r.paths.shape == (m, 6, 3)
    assert sum(r.counts.values()) == m
    for a, b in zip(_fields(r), _fields(whole)):
        assert a.tobytes() == np.ascontiguousarray(b[:m]).tobytes()
    if m == 0:
        d = pp.trace_pathlines(_velocity(case, U, device=True), torch.zeros((0, 3), dtype=torch.float64).cuda(), dt, max_steps)
        assert d.end.is_cuda and d.end.shape == (0, 3) and d.steps.shape == (0,) and sum(d.counts.values()) == 0


@pytest.mark.parametrize("case", TR.CASES, ids=IDS)
def test_path_record(case):
    U, S, _ = _smooth(case)
    dt, max_steps, min_speed = TR.configs(case[0])[1]
    r_every = 10
    f = _velocity(case, U)
    r = pp.trace_pathlines(f, S, dt, max_steps, min_speed=min_speed, record_every=r_every, chunk=7)
    assert r.paths.shape == (len(S), max_steps // r_every + 1, S.shape[1])
    inside = r.status != P.OUTSIDE
    assert np.array_equal(r.paths[inside, 0], S[inside]) and np.isnan(r.paths[~inside]).all()
    for j in (1, 2):
        t = pp.trace_pathlines(f, S, dt, j * r_every, min_speed=min_speed)
        reached = inside & (r.steps >= j * r_every)
        assert reached.sum() > 100 and (~reached).sum() > 100
        assert r.paths[reached, j].tobytes() == t.end[reached].tobytes()
        assert np.isnan(r.paths[~reached, j]).all()


@pytest.mark.parametrize("case", (TR.CASES[0], TR.CASES[3]), ids=(IDS[0], IDS[3]))
def test_device_in_device_out(case):
    U, S, _ = _smooth(case)
    dt, max_steps, min_speed = TR.configs(case[0])[1]
    host = pp.trace_pathlines(_velocity(case, U), S, dt, max_steps, min_speed=min_speed, record_every=5)
    fdev = _velocity(case, U, device=True)
    Sd = torch.from_numpy(S.copy()).cuda()
    before = dict(_ffi.fetch_stats)
    dev = pp.trace_pathlines(fdev, Sd, dt, max_steps, min_speed=min_speed, record_every=5)
    assert all(a.is_cuda for a in (dev.end, dev.time, dev.length, dev.steps, dev.status, dev.side, dev.paths))
    assert fdev.on_device and _ffi.fetch_stats == before
    assert dev.paths.shape == host.paths.shape and dev.counts == host.counts
    moved = P(*(a.cpu().numpy() for a in (dev.end, dev.time, dev.length, dev.steps, dev.status, dev.side, dev.paths)),
              dev.counts)
    assert _same_bits(host, moved)
    # host seeds on a device velocity: NumPy results, the velocity stays where it is
    mixed = pp.trace_pathlines(fdev, S, dt, max_steps, min_speed=min_speed, record_every=5)
    assert all(isinstance(a, np.ndarray) for a in _fields(mixed)) and isinstance(mixed.paths, np.ndarray)
    assert fdev.on_device and _ffi.fetch_stats == before and _same_bits(host, mixed)
    # device seeds on a host velocity: device results
    dev2 = pp.trace_pathlines(_velocity(case, U), Sd, dt, max_steps, min_speed=min_speed)
    assert dev2.end.is_cuda and np.array_equal(dev2.end.cpu().numpy(), host.end, equal_nan=True)


@pytest.mark.parametrize("case", (TR.CASES[2], TR.CASES[3]), ids=(IDS[2], IDS[3]))
def test_travel_times_of_a_linear_pressure(case):
    """p = 1 - x: the projected velocity is (k, 0, 0) at every node to the 1e-13 tolerance of the mass-matrix solve, so the
    travel time from x0 is (1 - x0) phi / k through side 2, and backwards x0 phi / k through side 1, to that tolerance
    (relative, times the few hundred steps that each carry it)."""
    kind, nx, ny, nz = case
    k, phi = 2.0, 0.25
    mesh = _space(case).mesh()
    p = fd.Function(fd.FunctionSpace(mesh, "CG", 1)).interpolate(lambda X: 1.0 - X[:, 0])
    u = pp.calculate_darcy_velocity_from_pressure(p, k)
    un = np.asarray(u.vector()).reshape(-1, 3)
    # The mass-matrix solves run to rtol 1e-13 (include/perphil_hip.h) on the residual: |u - u*|_2 <= cond(M) 1e-13 |u*|_2 with
    # |u*|_2 = k sqrt(n) and cond(M) <= (d + 2) * (largest / smallest nodal patch) = 5 * 24 on these meshes (27 for Q1).
    n = un.shape[0]
    tol_u = 1e-13 * 120 * np.sqrt(n) * k
    du = np.abs(un - np.array([k, 0.0, 0.0])).max()
    print(f"{TR.NAMES[kind]}: projected velocity, worst nodal error {du:.3g} (1e-13 solve tolerance allows {tol_u:.3g})")
    assert du <= tol_u
    X0 = 0.1 + 0.8 * np.random.default_rng(9).random((65, 3))
    dt = 1.0 / 1024
    fw = pp.travel_times(p, k, X0, dt, 1000, porosity=phi)
    assert (fw.status == P.EXITED).all() and (fw.side == 2).all() and fw.counts["exited"] == 65
    want = (1 - X0[:, 0]) * phi / k
    rel = tol_u / k + 4 * 2.0 ** -53 * fw.steps        # the velocity's relative error, and a few roundings per step
    print(f"{TR.NAMES[kind]}: forward travel time, worst relative error {(np.abs(fw.time - want) / want).max():.3g} "
          f"(allowed {rel.min():.3g})")
    assert (np.abs(fw.time - want) <= rel * want).all()
    drift = tol_u / phi * want + 4 * 2.0 ** -53 * fw.steps
    assert (fw.end[:, 0] == 1.0).all() and (np.abs(fw.end[:, 1:] - X0[:, 1:]) <= drift[:, None]).all()
    bw = pp.travel_times(p, k, X0, dt, 1000, porosity=phi, backward=True)
    assert (bw.status == P.EXITED).all() and (bw.side == 1).all() and (bw.end[:, 0] == 0.0).all()
    wantb = X0[:, 0] * phi / k
    assert (np.abs(bw.time - wantb) <= (tol_u / k + 4 * 2.0 ** -53 * bw.steps) * wantb).all()
    # a device-resident pressure keeps the whole chain on the device
    pdev = fd.Function(p.function_space(), torch.from_numpy(np.asarray(p.vector()).copy()).cuda())
    before = dict(_ffi.fetch_stats)
    dv = pp.travel_times(pdev, k, torch.from_numpy(X0).cuda(), dt, 1000, porosity=phi)
    assert dv.time.is_cuda and _ffi.fetch_stats == before and np.array_equal(dv.time.cpu().numpy(), fw.time)


def test_edge_cases():
    case = TR.CASES[1]
    kind, nx, ny, nz = case
    U, S, _ = _smooth(case)
    f = _velocity(case, U)
    # an outside seed and a NaN seed in the middle of a wave: status 3, NaN outputs, the neighbours undisturbed
    X = S[:64].copy()
    clean = pp.trace_pathlines(f, X, 0.02, 100)
    X[17] = [1.0 + 1e-12, 0.5]
    X[40] = [0.5, np.nan]
    r = pp.trace_pathlines(f, X, 0.02, 100)
    bad = np.zeros(64, bool)
    bad[[17, 40]] = True
    assert (r.status[bad] == P.OUTSIDE).all() and (r.steps[bad] == 0).all() and (r.side[bad] == 0).all()
    assert np.isnan(r.end[bad]).all() and np.isnan(r.time[bad]).all() and np.isnan(r.length[bad]).all()
    for a, b in zip(_fields(r), _fields(clean)):
        assert a[~bad].tobytes() == b[~bad].tobytes()
    assert r.counts["outside"] == 2 and sum(r.counts.values()) == 64
    # min_speed above the field's maximum: everybody is stagnant where it stands
    speed = np.sqrt((U ** 2).sum(axis=1)).max()
    s = pp.trace_pathlines(f, S[:200], 0.02, 100, min_speed=2 * speed)
    assert (s.status == P.STAGNANT).all() and (s.steps == 0).all() and np.array_equal(s.end, S[:200])
    assert (s.time == 0).all() and (s.length == 0).all() and s.counts["stagnant"] == 200
    # m = 0
    e = pp.trace_pathlines(f, np.zeros((0, 2)), 0.02, 100, record_every=10)
    assert e.end.shape == (0, 2) and e.time.shape == (0,) and e.status.shape == (0,) and e.paths.shape == (0, 11, 2)
    assert e.counts == dict.fromkeys(pp._STATUS_NAMES, 0)
    # one point
    one = pp.trace_pathlines(f, [0.5, 0.5], 0.02, 100)
    assert one.end.shape == (1, 2) and one.status[0] == P.EXITED


def test_library_refusals():
    """The C entry points refuse what the Python layer would let through only by mistake (PPH_ERR_INVALID, message)."""
    case = TR.CASES[0]
    U, S, _ = _smooth(case)
    ctx = _space(case).mesh().context()
    u = np.ascontiguousarray(U).reshape(-1)
    for kw, word in ((dict(dt=0.0), "dt"), (dict(dt=float("inf")), "dt"), (dict(scale=0.0), "scale"),
                     (dict(scale=float("nan")), "scale"), (dict(max_steps=0), "max_steps"), (dict(chunk=0), "chunk"),
                     (dict(record_every=-1), "record_every"), (dict(min_speed=-1.0), "min_speed"),
                     (dict(min_speed=float("nan")), "min_speed")):
        a = dict(scale=1.0, dt=0.1, max_steps=10, min_speed=0.0, chunk=4, record_every=0)
        a.update(kw)
        rec = a.pop("record_every")
        with pytest.raises(ValueError, match=word):
            ctx.trace_pathlines(u, S[:4], a["scale"], a["dt"], a["max_steps"], a["min_speed"], a["chunk"], rec)
    mesh2 = fd.Mesh(2, TR.QUAD, 3, 2, 0, comm=fd.COMM_SELF)
    ctx2 = mesh2.context(degree=2)
    with pytest.raises(ValueError, match="CG-1"):
        ctx2.trace_pathlines(np.zeros(ctx2.n * 2), S[:4], 1.0, 0.1, 10)
