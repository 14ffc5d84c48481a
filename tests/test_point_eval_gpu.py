"""Point evaluation on the device (pph_eval_points, Function.at / gradient_at, slice_along_x between grid lines) against
the longdouble restatement of tests/point_eval_reference.py, on all four cell kinds and degrees 1 and 2.

The bound, everywhere (point_eval_reference.value_bound / gradient_bound, where gamma is counted):
    |v_gpu - v_ref| <= 2^-53 (gamma S + sum_e n_e G_e)
    |g_gpu - g_ref|_e <= 2^-53 n_e (gamma_g G_e + sum_f n_f H_ef)      (points further than 1e-6 from every face)
Every test prints its worst ratio error / bound before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import perphil_amd as pa  # noqa: E402
from perphil_amd import _ffi, fd, postprocessing as pp, solver_parameters as spar  # noqa: E402
import point_eval_reference as PR  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
KD = [(c, deg) for c in PR.CASES for deg in (1, 2)]
IDS = [f"{('quad', 'tri', 'hex', 'tet')[c[0]]}-deg{deg}" for c, deg in KD]


def _mesh(kind, nx, ny, nz):
    return fd.Mesh(PR.dim_of(kind), kind, nx, ny, nz, comm=fd.COMM_SELF)


def _function(kind, deg, nx, ny, nz, u):
    mesh = _mesh(kind, nx, ny, nz)
    return fd.Function(fd.FunctionSpace(mesh, "CG", deg), np.ascontiguousarray(u, dtype=np.float64).reshape(-1).copy())


def _worst(err, bound, what):
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    ratio = np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD(1e-300)))
    k = int(np.argmax(ratio))
    print(f"{what}: worst error / bound = {float(ratio.ravel()[k]):.3f} at flat index {k} (error {float(err.ravel()[k]):.3e}, "
          f"bound {float(bound.ravel()[k]):.3e}) over {err.size} entries")
    return float(ratio.ravel()[k])


@pytest.mark.parametrize("case,deg", KD, ids=IDS)
def test_values_against_the_restatement(case, deg):
    kind, nx, ny, nz = case
    u = PR.random_coefficients(kind, deg, nx, ny, nz)
    X = np.concatenate([PR.random_points(kind, deg), PR.deliberate_points(kind, nx, ny, nz)])
    f = _function(kind, deg, nx, ny, nz, u)
    v = f.at(X)
    assert v.shape == (len(X),) and not np.isnan(v).any()
    ref = PR.evaluate(kind, deg, nx, ny, nz, u, X)
    err = np.abs(v.astype(LD) - ref["v"][:, 0])
    assert _worst(err, PR.value_bound(kind, deg, nx, ny, nz, ref)[:, 0], f"values {IDS[KD.index((case, deg))]}") <= 1.0


@pytest.mark.parametrize("case,deg", KD, ids=IDS)
def test_interpolated_polynomials_are_evaluated_exactly(case, deg):
    """interpolate() of a polynomial of the space whose nodal values are integers (no rounding in the coefficients), then at()
    against the polynomial itself under the same bound."""
    kind, nx, ny, nz = case
    n = PR.boxes(kind, nx, ny, nz)
    poly = PR.integer_polynomial(kind, deg, nx, ny, nz)
    mesh = _mesh(kind, nx, ny, nz)
    f = fd.Function(fd.FunctionSpace(mesh, "CG", deg)).interpolate(lambda Y: poly(np.rint(Y * (deg * n))))
    X = PR.random_points(kind, deg)
    v = f.at(X)
    exact = poly(X.astype(LD) * (deg * n).astype(LD))
    ref = PR.evaluate(kind, deg, nx, ny, nz, f.vector(), X)
    err = np.abs(v.astype(LD) - exact)
    assert _worst(err, PR.value_bound(kind, deg, nx, ny, nz, ref)[:, 0], "polynomial") <= 1.0


@pytest.mark.parametrize("case,deg", KD, ids=IDS)
def test_gradients_against_the_restatement(case, deg):
    kind, nx, ny, nz = case
    d = PR.dim_of(kind)
    u = PR.random_coefficients(kind, deg, nx, ny, nz)
    X = PR.random_points(kind, deg)
    keep = PR.face_distance(kind, nx, ny, nz, X) > 1e-6
    assert np.count_nonzero(~keep) <= 0.01 * len(X)          # (asserted for these seeds on the CPU as well)
    f = _function(kind, deg, nx, ny, nz, u)
    g = f.gradient_at(X)
    assert g.shape == (len(X), d)
    ref = PR.evaluate(kind, deg, nx, ny, nz, u, X[keep])
    err = np.abs(g[keep].astype(LD) - ref["g"][:, 0])
    assert _worst(err, PR.gradient_bound(kind, deg, nx, ny, nz, ref)[:, 0], "gradients") <= 1.0
    # a single point: [dim]
    g1 = f.gradient_at(tuple(X[0]))
    assert g1.shape == (d,) and np.array_equal(g1, g[0])


@pytest.mark.parametrize("case,deg", [KD[1], KD[6]], ids=[IDS[1], IDS[6]])
def test_device_points_on_a_device_function_stay_on_the_device(case, deg):
    kind, nx, ny, nz = case
    u = PR.random_coefficients(kind, deg, nx, ny, nz)[:, 0]
    X = PR.random_points(kind, deg, 500)
    host = _function(kind, deg, nx, ny, nz, u)
    v_host, g_host = host.at(X), host.gradient_at(X)
    mesh = _mesh(kind, nx, ny, nz)
    fdev = fd.Function(fd.FunctionSpace(mesh, "CG", deg), torch.from_numpy(u.copy()).cuda())
    before = dict(_ffi.fetch_stats)
    Xd = torch.from_numpy(X).cuda()
    v, g = fdev.at(Xd), fdev.gradient_at(Xd)
    assert v.is_cuda and g.is_cuda and fdev.on_device and _ffi.fetch_stats == before
    assert np.array_equal(v.cpu().numpy(), v_host) and np.array_equal(g.cpu().numpy(), g_host)
    # host points on the device function: only points and results move
    v2 = fdev.at(X)
    assert isinstance(v2, np.ndarray) and np.array_equal(v2, v_host) and fdev.on_device and _ffi.fetch_stats == before
    # device points on a host function: a device tensor as well
    v3 = host.at(Xd)
    assert v3.is_cuda and np.array_equal(v3.cpu().numpy(), v_host)
    # a single off-lattice point is a float from the kernel
    s = fdev.at(tuple(X[3]))
    assert isinstance(s, float) and s == v_host[3] and fdev.on_device


def test_solved_subfunctions_mixed_and_vector_functions():
    params = pa.DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
    mesh = fd.UnitSquareMesh(12, 10, quadrilateral=True)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    _, p1, _, p2 = pa.exact_expressions(mesh, params)
    sol = pa.solve_dpp(W, params, [fd.DirichletBC(W.sub(0), p1), fd.DirichletBC(W.sub(1), p2)],
                       solver_parameters=spar.FIELDSPLIT_MG_PARAMS)
    X = np.random.default_rng(3).random((300, 2))
    parts = [sol.solution.sub(i).at(X) for i in range(2)]
    both = sol.solution.at(X)
    assert isinstance(both, tuple) and len(both) == 2
    full = sol.solution.vector().reshape(2, -1)
    for i in range(2):
        assert np.array_equal(both[i], parts[i])
        ref = PR.evaluate(PR.QUAD, 1, 12, 10, 0, full[i], X)
        err = np.abs(parts[i].astype(LD) - ref["v"][:, 0])
        assert _worst(err, PR.value_bound(PR.QUAD, 1, 12, 10, 0, ref)[:, 0], f"solved sub({i})") <= 1.0
    one = sol.solution.at(tuple(X[0]))
    assert isinstance(one, tuple) and one == (parts[0][0], parts[1][0])
    # the Darcy velocity of the CG-1 pressure: a vector function, [m, dim], column = that component alone
    p1h = fd.Function(V, full[0].copy())
    vel = pp.calculate_darcy_velocity_from_pressure(p1h, 1.0)
    uv = vel.at(X)
    assert uv.shape == (300, 2)
    comp = vel.vector().reshape(-1, 2)
    for c in range(2):
        assert np.array_equal(uv[:, c], fd.Function(V, comp[:, c].copy()).at(X))
    gv = vel.gradient_at(X)
    assert gv.shape == (300, 2, 2)
    assert np.array_equal(gv[:, 1], fd.Function(V, comp[:, 1].copy()).gradient_at(X))
    ref = PR.evaluate(PR.QUAD, 1, 12, 10, 0, comp, X)
    err = np.abs(uv.astype(LD) - ref["v"])
    assert _worst(err, PR.value_bound(PR.QUAD, 1, 12, 10, 0, ref), "vector function") <= 1.0


@pytest.mark.parametrize("deg", (1, 2))
@pytest.mark.parametrize("kind", (PR.QUAD, PR.TRI))
def test_lattice_points_and_grid_line_slices_are_the_coefficients(kind, deg):
    nx, ny = 8, 6
    u = PR.random_coefficients(kind, deg, nx, ny, 0)[:, 0]
    f = _function(kind, deg, nx, ny, 0, u)
    px = deg * nx + 1
    for (i, j) in ((0, 0), (3, 2), (deg * nx, deg * ny), (1, deg * ny - 1)):
        assert f.at((i / (deg * nx), j / (deg * ny))) == u[i + px * j]
    y, vals = pp.slice_along_x(f, 0.5)
    i = deg * nx // 2
    direct = np.array([u[i + px * (deg * j)] for j in range(ny + 1)])
    assert np.array_equal(y, np.arange(ny + 1) / ny) and np.array_equal(vals, direct)
    mesh = _mesh(kind, nx, ny, 0)
    fdev = fd.Function(fd.FunctionSpace(mesh, "CG", deg), torch.from_numpy(u.copy()).cuda())
    assert np.array_equal(pp.slice_along_x(fdev, 0.5)[1], direct) and fdev.on_device


@pytest.mark.parametrize("deg", (1, 2))
@pytest.mark.parametrize("kind", (PR.QUAD, PR.TRI))
def test_slices_between_grid_lines(kind, deg):
    nx, ny = 7, 5
    u = PR.random_coefficients(kind, deg, nx, ny, 0)[:, 0]
    f = _function(kind, deg, nx, ny, 0, u)
    mesh = _mesh(kind, nx, ny, 0)
    fdev = fd.Function(fd.FunctionSpace(mesh, "CG", deg), torch.from_numpy(u.copy()).cuda())
    for xv in (0.3, 0.5, 0.999, 1.0 / 3.0):
        y, vals = pp.slice_along_x(f, xv)
        X = np.stack([np.full(ny + 1, xv), y], axis=1)
        ref = PR.evaluate(kind, deg, nx, ny, 0, u, X)
        err = np.abs(vals.astype(LD) - ref["v"][:, 0])
        assert _worst(err, PR.value_bound(kind, deg, nx, ny, 0, ref)[:, 0], f"slice x = {xv}") <= 1.0
        yd, vd = pp.slice_along_x(fdev, xv)
        assert np.array_equal(vd, vals) and fdev.on_device


@pytest.mark.parametrize("case,deg", [KD[0], KD[3], KD[5], KD[6]], ids=[IDS[0], IDS[3], IDS[5], IDS[6]])
def test_outside_points(case, deg):
    kind, nx, ny, nz = case
    d = PR.dim_of(kind)
    u = PR.random_coefficients(kind, deg, nx, ny, nz)[:, 0]
    f = _function(kind, deg, nx, ny, nz, u)
    rng = np.random.default_rng(11)
    X = rng.random((400, d))
    bad = np.sort(rng.choice(400, 37, replace=False))
    X[bad, rng.integers(0, d, 37)] = rng.choice([-0.25, 1.5, 1.0 + 1e-9, -1e-10, np.nan], 37)
    with pytest.raises(fd.PointNotInDomainError) as e:
        f.at(X)
    assert f"index {bad[0]}" in str(e.value)
    with pytest.raises(fd.PointNotInDomainError):
        f.at(torch.from_numpy(X).cuda())
    inside = np.setdiff1d(np.arange(400), bad)
    clean = f.at(X[inside])
    v = f.at(X, dont_raise=True)
    g = f.gradient_at(X, dont_raise=True)
    assert np.array_equal(np.nonzero(np.isnan(v))[0], bad) and np.array_equal(v[inside], clean)
    assert np.array_equal(np.nonzero(np.isnan(g).all(axis=1))[0], bad) and not np.isnan(g[inside]).any()
    ctx = pp._context(f)
    val, grad, nout = ctx.eval_points(u, X, gradient=True)
    assert nout == len(bad) == np.count_nonzero(np.isnan(val[:, 0])) and np.array_equal(val[:, 0], v, equal_nan=True)
    vd = f.at(torch.from_numpy(X).cuda(), dont_raise=True)
    assert vd.is_cuda and np.array_equal(vd.cpu().numpy(), v, equal_nan=True)
    # a wider tolerance takes the nearly-inside points in (clamped onto the boundary)
    wide = f.at(X, dont_raise=True, tolerance=1e-6)
    assert np.count_nonzero(np.isnan(wide)) < len(bad)


SCALE = [(PR.HEX, 1, 128, 128, 128), (PR.HEX, 2, 64, 64, 64), (PR.TET, 2, 64, 64, 48)]


@pytest.mark.parametrize("kind,deg,nx,ny,nz", SCALE, ids=["hex128-deg1", "hex64-deg2", "tet64x64x48-deg2"])
def test_four_million_points(kind, deg, nx, ny, nz):
    """More points than any grid cap (8192 workgroups of 256): the grid-stride loop; every point against the vectorised
    restatement under the same bound."""
    m = 1 << 22
    rng = np.random.default_rng(100 + kind + deg)
    n = PR.n_nodes(kind, deg, nx, ny, nz)
    u = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
    X = rng.random((m, 3))
    mesh = _mesh(kind, nx, ny, nz)
    f = fd.Function(fd.FunctionSpace(mesh, "CG", deg), u)
    v = f.at(X)
    assert v.shape == (m,) and not np.isnan(v).any()
    worst = 0.0
    for b0 in range(0, m, 1 << 20):
        sl = slice(b0, b0 + (1 << 20))
        ref = PR.evaluate_fast(kind, deg, nx, ny, nz, u, X[sl], gradient=False)
        err = np.abs(v[sl].astype(LD) - ref["v"][:, 0])
        worst = max(worst, _worst(err, PR.value_bound(kind, deg, nx, ny, nz, ref)[:, 0], f"scale points {b0}.."))
    assert worst <= 1.0
