"""Wells and distributed sources of the transient runs on the device (perphil_amd/csrc/pph_sources.hip, the source hooks of
pph_transient.hip and pph_transient_adjoint.hip, perphil_amd/transient.py) against the restatement of
tests/transient_sources_reference.py.

Bars.
  sources_apply: every entry within APPLY_BAR ulp of sum_k |c_k| |L_k| (the manner of transient_reference.abs_bound): ten times
      the worst ratio measured over this file's cases (APPLY_MEASURED: 2.89, degree-2 tetrahedra with 1036 points; the other
      shapes 0.37 to 1.68, the 1024 x 512 mesh 1.93); a wrong basis value or a dropped point shows at 1e-2 of that scale,
      thirteen decades above the bar.
  stepping: the final state against the restatement's direct (splu) stepping, relative to max |p|, all solves to rtol 1e-12:
      SRC_STEP_TOL, ten times the worst value measured over this file's cases (SRC_STEP_MEASURED: 1.29e-13, quadrilaterals 5 x 3
      under CG + Jacobi at theta 1; the other stepping cases 1.8e-16 to 1.1e-13, the closed form 8.3e-16, the pumping test
      1.8e-14) - the protocol of STEP_TOL in tests/test_transient_gpu.py; it stays below 1e-10, and a wrong coefficient shows
      at 1e-2.
  rate gradients: src_grad against the restatement's G, of their absolute sums |w_s|^T |F L_k|: the protocol of the `terms` in
      tests/test_transient_adjoint_gpu.py - the larger of 1e-10 and ten times what the restatement itself loses when its solves
      run by the oracle's pcg at rtol 1e-13 instead of splu (SRC_GRAD_CPU_MEASURED, measured on the CPU over the runs of this
      file); ten times that is below 1e-10, so the bar is 1e-10, as LOOP_BAR there.
Every test prints its worst figure before it asserts."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import dpp_oracle as o  # noqa: E402
from perphil_amd import _ffi, solver_parameters as spar  # noqa: E402
import point_eval_reference as PE  # noqa: E402
import test_transient_gpu as TG  # noqa: E402
import transient_adjoint_reference as A  # noqa: E402
import transient_reference as T  # noqa: E402
import transient_sources_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

CF = TG.CF
APPLY_MEASURED = 2.89         # worst |b - ref| / (eps sum |c_k| |L_k|) over the cases of test_sources_apply_* and the large mesh
APPLY_BAR = 10 * APPLY_MEASURED
SRC_STEP_MEASURED = 1.29e-13  # worst final-state error over the stepping, closed-form and pumping-test cases of this file
SRC_STEP_TOL = 10 * SRC_STEP_MEASURED
SRC_GRAD_CPU_MEASURED = 1.69e-12   # tools/transient_sources_cpu_loss.py: the five degree-1 runs of STEP_RUNS, both theta (no GPU needed)
SRC_GRAD_DEVICE_MEASURED = 7.94e-12   # worst src_grad figure the device gave over the gradient cases of this file (degree-2 quadrilaterals, theta 1/2)
SRC_GRAD_BAR = max(1e-10, 10 * SRC_GRAD_CPU_MEASURED)
LOOP_BAR = 1e-10              # tests/test_transient_adjoint_gpu.py: terms, q0 of the backward loop
PASS_PAIRS = 2048 * 256       # pairs of entries one pass of k_src_dense's grid covers (SRC_MAX_BLOCKS x 256)

APPLY_CASES = [(o.CELL_QUAD, 5, 3, 0, 1), (o.CELL_TRI, 4, 3, 0, 1), (o.CELL_HEX, 3, 4, 2, 1), (o.CELL_TET, 3, 2, 3, 1),
               (o.CELL_QUAD, 4, 4, 0, 2), (o.CELL_TET, 2, 2, 2, 2)]


def _cid(c):
    return f"{TG.NAMES[c[0]]}{c[1]}x{c[2]}x{c[3]}-deg{c[4]}"


def _spread(rng, size):
    return rng.standard_normal(size) * 10.0 ** rng.uniform(-2, 2, size)


@functools.lru_cache(maxsize=None)
def _mesh_data(kind, nx, ny, nz, degree):
    """(n, K, M, coordinates, boundary nodes) of a mesh: the oracle's at degree 1, the context's own export at degree 2."""
    if degree == 1:
        om, K, M = T.scalar_matrices(TG._dim(kind), kind, nx, ny, nz)
        return om.num_nodes, K, M, om.coords, o.boundary_nodes(om)
    import p2_restatement as R2

    probe = _ffi.Context(0)
    probe.mesh_build_lagrange(TG._dim(kind), kind, nx, ny, nz, degree)
    K, M = probe.csr(_ffi.MAT_K), probe.csr(_ffi.MAT_M)
    n = probe.n
    probe.close()
    return n, K, M, R2.coords(kind, nx, ny, nz), R2.boundary_nodes(kind, nx, ny, nz)


def _sets(kind, nx, ny, nz, degree, which):
    n, _, _, X, bnd = _mesh_data(kind, nx, ny, nz, degree)
    if which == "none":
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if which == "shared":
        return bnd, bnd
    if degree == 1:
        return TG._dirichlet_sets(kind, nx, ny, nz, "mixed")
    inner = np.setdiff1d(np.arange(n), bnd)
    return bnd, np.sort(np.concatenate([bnd[(X[bnd, 0] < 1e-12) | (X[bnd, 1] < 1e-12)], inner[::7]]))


def _context(make, kind, nx, ny, nz, degree, nodes, g=None):
    ctx = make()
    if degree == 1:
        ctx.mesh_build(TG._dim(kind), kind, nx, ny, nz)
    else:
        ctx.mesh_build_lagrange(TG._dim(kind), kind, nx, ny, nz, degree)
    rng = np.random.default_rng(5)
    for f in (0, 1):
        ctx.set_dirichlet(f, nodes[f], rng.standard_normal(len(nodes[f])) if g is None else g[f][nodes[f]])
    return ctx


def _apply_points(kind, nx, ny, nz, degree, nodes):
    """Interior points, points on faces, edges and vertices (deliberate_points), on the domain boundary and its corners, two
    points in one cell, two identical points, one on a constrained node (a node of field 0's set, in network 0), one outside
    (the last)."""
    dim = TG._dim(kind)
    _, _, _, X, _ = _mesh_data(kind, nx, ny, nz, degree)
    rnd = PE.random_points(kind, degree, 12)
    h = 1.0 / np.array([nx, ny, nz][:dim])
    centre = 0.5 * h                                      # box 0: two points in one cell
    on_node = X[nodes[0][len(nodes[0]) // 2]] if len(nodes[0]) else X[len(X) // 2]
    edge_mid = np.array([0.5] + [0.0] * (dim - 1))
    pts = np.concatenate([rnd, PE.deliberate_points(kind, nx, ny, nz), np.zeros((1, dim)), np.ones((1, dim)), edge_mid[None],
                          (centre - 0.1 * h)[None], (centre - 0.2 * h)[None], rnd[1:2], rnd[1:2], on_node[None],
                          np.array([[1.5] + [0.5] * (dim - 1)])])
    fields = (np.arange(len(pts)) % 2).astype(np.int32)
    fields[-2] = 0
    return np.ascontiguousarray(pts), fields


@pytest.mark.parametrize("sets", ["none", "shared", "mixed"])
@pytest.mark.parametrize("case", APPLY_CASES, ids=_cid)
def test_sources_apply_matches_the_restatement(gpu_ctx_factory, case, sets):
    kind, nx, ny, nz, degree = case
    n, K, M, X, bnd = _mesh_data(kind, nx, ny, nz, degree)
    nodes = _sets(kind, nx, ny, nz, degree, sets)
    masks = T.masks_of(n, *nodes)
    con = np.concatenate(masks)
    pts, fields = _apply_points(kind, nx, ny, nz, degree, nodes)
    m = len(pts)
    rng = np.random.default_rng(40 + APPLY_CASES.index(case))
    dense = rng.standard_normal((2, 2 * n))
    Lp, outside = S.point_loads(kind, degree, nx, ny, nz, pts, fields)
    assert outside[-1] and not outside[:-1].any()
    loads = np.concatenate([dense, Lp])
    ctx = _context(gpu_ctx_factory, kind, nx, ny, nz, degree, nodes)
    assert ctx.n == n and ctx.sources_count() == -1
    assert ctx.sources_set(dense, pts, fields) == 1 and ctx.sources_count() == 2 + m
    # (coefficients and dense loads of magnitude 1: the basis values of a point carry ABSOLUTE rounding errors of a few eps - the
    #  box-local coordinate is a difference of numbers up to the box count - so the sum they are measured against must not be tiny)
    c = rng.standard_normal(2 + m)
    zero = np.zeros(2 * n)
    ref, mag = S.apply_loads(zero, loads, c, masks)
    got = ctx.sources_apply(c, zero.copy())
    ratio = float((np.abs(got - ref) / np.maximum(mag, 1e-300)).max() / T.EPS)
    print(f"{_cid(case)} {sets}: worst |b - ref| / (eps sum |c||L|) = {ratio:.2f} (bar {APPLY_BAR:g}), {m} points, {int(con.sum())} constrained dofs")
    assert np.all(np.abs(got - ref) <= APPLY_BAR * T.EPS * mag)
    assert np.all(got[con] == 0.0) and np.count_nonzero(got) == int((~con).sum())
    # onto a non-zero b: the same sum added once, constrained entries untouched bit for bit
    b0 = _spread(rng, 2 * n)
    b = ctx.sources_apply(c, b0.copy())
    assert np.array_equal(b[con], b0[con]) and np.all(np.abs(b - (b0 + got)) <= 2 * T.EPS * (np.abs(b0) + np.abs(got)))
    # two calls, the device variant of set and apply, a zero row, and the outside point's empty row
    assert np.array_equal(b, ctx.sources_apply(c, b0.copy()))
    assert np.array_equal(b0, ctx.sources_apply(np.zeros(2 + m), b0.copy()))
    only_outside = np.zeros(2 + m)
    only_outside[-1] = 7.0
    assert np.array_equal(b0, ctx.sources_apply(only_outside, b0.copy()))
    bd = ctx.sources_apply(c, torch.from_numpy(b0.copy()).cuda())
    odd = torch.zeros(2 * n + 1, dtype=torch.float64, device="cuda")[1:]      # 8-byte aligned only: the 8-byte accesses, the same bits
    odd.copy_(torch.from_numpy(b0))
    assert odd.data_ptr() % 16 == 8 and np.array_equal(ctx.sources_apply(c, odd).cpu().numpy(), b)
    assert bd.is_cuda and np.array_equal(bd.cpu().numpy(), b)
    dev = _context(gpu_ctx_factory, kind, nx, ny, nz, degree, nodes)
    assert dev.sources_set(torch.from_numpy(dense).cuda(), torch.from_numpy(pts).cuda(), fields) == 1
    assert np.array_equal(dev.sources_apply(c, b0.copy()), b)
    # every point alone is its restated load; the dense part alone and the point part alone (either part skipped when empty)
    for p in (0, m - 5, m - 4, m - 3, m - 2):
        e = np.zeros(2 + m)
        e[2 + p] = 1.0
        one = ctx.sources_apply(e, zero.copy())
        assert np.all(np.abs(one - np.where(con, 0.0, Lp[p])) <= APPLY_BAR * T.EPS), p      # (basis values: magnitude <= 1)
    # the well on a constrained node pumps into the boundary condition: nothing but rounding-size weights of its neighbours
    assert np.abs(ctx.sources_apply(np.eye(2 + m)[2 + m - 2], zero.copy())).max() <= 1e-14 or sets == "none"
    assert dev.sources_set(dense, None, None) == 0 and dev.sources_count() == 2
    assert np.all(np.abs(dev.sources_apply(c[:2], zero.copy()) - S.apply_loads(zero, dense, c[:2], masks)[0]) <= APPLY_BAR * T.EPS * mag)
    assert dev.sources_set(None, pts, fields) == 1 and dev.sources_count() == m
    assert np.all(np.abs(dev.sources_apply(c[2:], zero.copy()) - S.apply_loads(zero, Lp, c[2:], masks)[0]) <= APPLY_BAR * T.EPS * mag)
    dev.sources_clear()
    assert dev.sources_count() == -1
    with pytest.raises(ValueError, match="no source set"):
        dev.sources_apply(c, zero.copy())
    # a mesh build clears the set
    if degree == 1:
        ctx.mesh_build(TG._dim(kind), kind, nx, ny, nz)
        assert ctx.sources_count() == -1


def test_more_entries_than_one_pass_of_the_dense_grid(gpu_ctx_factory):
    """1024 x 512 quadrilaterals: 2n = 1 051 650 entries, 525 825 pairs; the 2048 workgroups of k_src_dense cover 524 288
    pairs per pass.  Three dense loads and four wells (one at the last node), against NumPy."""
    kind, nx, ny = o.CELL_QUAD, 1024, 512
    n = (nx + 1) * (ny + 1)
    assert n > PASS_PAIRS
    idx = np.arange(n)
    i, j = idx % (nx + 1), idx // (nx + 1)
    b0n = idx[(i == 0) | (i == nx) | (j == 0)]
    b1n = idx[(i == 0) | ((i == 400) & (j == ny - 1)) | (idx == n - 3)]      # (constrained dofs in the second pass too)
    masks = T.masks_of(n, b0n, b1n)
    con = np.concatenate(masks)
    rng = np.random.default_rng(12)
    dense = rng.standard_normal((3, 2 * n))
    pts = np.array([[1.0, 1.0], [1.0 - 0.25 / nx, 1.0 - 0.5 / ny], [0.3, 0.7], [0.0, 0.0]])
    fields = np.array([1, 1, 0, 0], dtype=np.int32)
    ctx = _context(gpu_ctx_factory, kind, nx, ny, 0, 1, (b0n, b1n))
    assert ctx.sources_set(dense, pts, fields) == 0
    c = rng.standard_normal(7)
    b0 = rng.standard_normal(2 * n)
    b = ctx.sources_apply(c, b0.copy())
    E, outside = A.point_matrix(kind, 1, nx, ny, 0, pts)
    assert not outside.any()
    Lp = np.zeros((4, 2 * n))
    for q in range(4):
        Lp[q, fields[q] * n:(fields[q] + 1) * n] = E[q].toarray()[0]
    assert Lp[0, 2 * n - 1] == 1.0 and Lp[3, 0] == 1.0 and Lp[1, n + nx + (nx + 1) * (ny - 1)] == 0.375      # (powers of two: exact)
    add = c[:3] @ dense + c[3:] @ Lp
    mag = np.abs(c[:3]) @ np.abs(dense) + np.abs(c[3:]) @ np.abs(Lp)
    ref = np.where(con, b0, b0 + add)
    ratio = float((np.abs(b - ref) / (mag + np.abs(b0))).max() / T.EPS)
    print(f"quad1024x512: worst |b - ref| / (eps (sum |c||L| + |b|)) = {ratio:.2f} (bar {APPLY_BAR:g})")
    assert np.all(np.abs(b - ref) <= APPLY_BAR * T.EPS * (mag + np.abs(b0)))
    assert np.array_equal(b[con], b0[con]) and np.count_nonzero((b != b0)[2 * PASS_PAIRS:]) > 1000      # the second pass did its share
    assert np.array_equal(b, ctx.sources_apply(c, b0.copy()))
    assert np.array_equal(b, ctx.sources_apply(c, torch.from_numpy(b0.copy()).cuda()).cpu().numpy())


# ---- the step loop ---------------------------------------------------------------------------------------------------------
STEP_RUNS = [((o.CELL_QUAD, 5, 3, 0), 1, "cg_jacobi"), ((o.CELL_HEX, 3, 4, 2), 1, "gmres_ilu"), ((o.CELL_HEX, 4, 4, 4), 1, "picard_mg"),
             ((o.CELL_TET, 4, 4, 4), 1, "cg_cmg"), ((o.CELL_QUAD, 8, 8, 0), 1, "fieldsplit_lu"), ((o.CELL_QUAD, 4, 4, 0), 2, "pmg")]
N_STEPS = 6
STORAGE, DT = (0.3, 5.0), 0.02


def _rid(i):
    r = STEP_RUNS[i]
    return f"{TG._id(r[0])}-deg{r[1]}-{r[2]}"


def _solver(run):
    (_, _, _, _), degree, name = run
    params, nonlinear = (spar.FIELDSPLIT_PMG_PARAMS, False) if degree == 2 else TG.SOLVERS[name]
    return TG._cfg(params, nonlinear)


@functools.lru_cache(maxsize=None)
def _step_problem(run_index, theta):
    """Matrices, Dirichlet sets and data, two wells (one per network) and two distributed sources (one per network) with rates that change every
    step, and the restatement's states: computed once per run and theta, shared by the stepping and the gradient tests."""
    (kind, nx, ny, nz), degree, name = STEP_RUNS[run_index]
    n, K, M, X, bnd = _mesh_data(kind, nx, ny, nz, degree)
    rng = np.random.default_rng(70 + run_index)
    if degree == 1:
        nodes = TG._dirichlet_sets(kind, nx, ny, nz, "mixed")
        p0 = TG._initial(o.build_mesh(TG._dim(kind), kind, nx, ny, nz), 2)
    else:
        nodes = (np.sort(rng.choice(n, n // 5, replace=False)), np.sort(rng.choice(n, n // 6, replace=False)))
        p0 = rng.standard_normal(2 * n)
    masks = T.masks_of(n, *nodes)
    g = TG._dirichlet_data(n, nodes, 6)
    dim = TG._dim(kind)
    pts = np.ascontiguousarray(np.array([[0.37, 0.61, 0.29], [0.5, 0.5, 0.5]])[:, :dim])      # (the second on a node / face of most meshes)
    fields = np.array([0, 1], dtype=np.int32)
    f = np.cos(2.0 * X[:, 0]) * (1.0 + X[:, 1])
    dense = np.stack([S.mass_load(M, f, 1), S.mass_load(M, np.sin(3.0 * X[:, -1]) - 0.2, 0)])      # (two: the load index of k_src_dot's grid)
    Lp, outside = S.point_loads(kind, degree, nx, ny, nz, pts, fields)
    assert not outside.any()
    loads = np.concatenate([dense, Lp])
    rates = rng.uniform(-2.0, 3.0, (N_STEPS + 1, 4))
    coef = S.coefficients(rates, theta)
    states, bn, dn = S.theta_steps(K, M, CF, STORAGE, theta, DT, masks, g, p0, N_STEPS, loads, coef)
    return dict(n=n, K=K, M=M, nodes=nodes, masks=masks, g=g, p0=p0, pts=pts, fields=fields, dense=dense, loads=loads, coef=coef,
                states=np.stack(states), bn=bn, dn=dn)


def _step_context(make, run, pr):
    (kind, nx, ny, nz), degree, _ = run
    ctx = _context(make, kind, nx, ny, nz, degree, pr["nodes"], pr["g"])
    assert ctx.sources_set(pr["dense"], pr["pts"], pr["fields"]) == 0
    return ctx


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("run", range(len(STEP_RUNS)), ids=_rid)
def test_stepping_with_sources_matches_the_restatement(gpu_ctx_factory, run, theta):
    pr = _step_problem(run, theta)
    cfg = _solver(STEP_RUNS[run])
    ctx = _step_context(gpu_ctx_factory, STEP_RUNS[run], pr)
    ctx.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, STORAGE, theta, DT, monolithic=not cfg.picard)
    p = pr["p0"].copy()
    done, infos, norms = ctx.transient_steps(cfg, p, N_STEPS, coef=pr["coef"])
    ref = pr["states"][-1]
    err = np.abs(p - ref).max() / np.abs(ref).max()
    plain = T.theta_steps(pr["K"], pr["M"], CF, STORAGE, theta, DT, pr["masks"], pr["g"], pr["p0"], N_STEPS)[0][-1]
    print(f"steps with sources {_rid(run)} theta {theta}: {err:.2e} (bar {SRC_STEP_TOL:.1e}); the run without sources differs by "
          f"{np.abs(plain - ref).max() / np.abs(ref).max():.1e}; iterations {[i.iterations for i in infos]}")
    assert done == N_STEPS and all(i.converged for i in infos)
    assert err <= SRC_STEP_TOL < 1e-10 and np.abs(plain - ref).max() > 1e-3 * np.abs(ref).max()
    assert np.allclose(norms[:, 0], pr["bn"], rtol=1e-8, atol=0) and np.allclose(norms[:, 1], pr["dn"], rtol=1e-8, atol=0)
    con = np.concatenate(pr["masks"])
    assert np.array_equal(p[con], np.concatenate(pr["g"])[con])
    # 3 + 3 = 6 bit for bit, the context's vectors restored, the recording and the device variants: the same bits
    before = ctx.rhs() + (ctx.solution().copy(),)
    q = pr["p0"].copy()
    d1, _, n1 = ctx.transient_steps(cfg, q, 3, coef=pr["coef"][:3])
    d2, _, n2 = ctx.transient_steps(cfg, q, 3, coef=pr["coef"][3:])
    assert d1 == d2 == 3 and np.array_equal(q, p) and np.array_equal(np.vstack([n1, n2]), norms)
    after = ctx.rhs() + (ctx.solution().copy(),)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    r = pr["p0"].copy()
    d3, _, n3, traj = ctx.transient_steps(cfg, r, N_STEPS, record=True, coef=pr["coef"])
    assert d3 == N_STEPS and np.array_equal(r, p) and np.array_equal(n3, norms) and np.array_equal(traj[-1], p)
    assert np.array_equal(traj[0], np.where(con, np.concatenate(pr["g"]), pr["p0"]))
    qd = torch.from_numpy(pr["p0"].copy()).cuda()
    d4, _, n4 = ctx.transient_steps(cfg, qd, N_STEPS, coef=pr["coef"])
    assert d4 == N_STEPS and np.array_equal(qd.cpu().numpy(), p) and np.array_equal(n4, norms)
    # all-zero rates reproduce pph_transient_steps bit for bit
    z, y = pr["p0"].copy(), pr["p0"].copy()
    dz, _, nz_ = ctx.transient_steps(cfg, z, N_STEPS, coef=np.zeros_like(pr["coef"]))
    dy, _, ny_ = ctx.transient_steps(cfg, y, N_STEPS)
    assert dz == dy == N_STEPS and np.array_equal(z, y) and np.array_equal(nz_, ny_)
    after = ctx.rhs() + (ctx.solution().copy(),)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("case", [(o.CELL_QUAD, 4, 4, 0), (o.CELL_HEX, 3, 3, 3)], ids=TG._id)
def test_a_sine_source_follows_the_closed_form(gpu_ctx_factory, case, theta):
    kind, nx, ny, nz = case
    dim = TG._dim(kind)
    om, K, M = T.scalar_matrices(dim, kind, nx, ny, nz)
    n = om.num_nodes
    b = o.boundary_nodes(om)
    phi = T.sine_mode(om)
    phi[b] = 0.0
    storage, dt, N = (1.0, 20.0), 0.05, 8
    rates = np.array([0.0, 1.0, -2.0, 0.5, 0.5, 3.0, 0.0, 1.5, -1.0])[:, None]
    coef = S.coefficients(rates, theta)
    amp = S.closed_form_source_amplitudes(dim, nx, ny, nz, CF, storage, theta, dt, (1.0, -0.5), coef[:, 0], 1)[-1]
    ctx = _context(gpu_ctx_factory, kind, nx, ny, nz, 1, (b, b), (np.zeros(n), np.zeros(n)))
    ctx.sources_set(S.mass_load(M, phi, 1)[None], None, None)
    ctx.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, storage, theta, dt)
    p = np.concatenate([phi, -0.5 * phi])
    done, infos, _ = ctx.transient_steps(TG._cfg(spar.CG_JACOBI_PARAMS), p, N, coef=coef)
    err = np.abs(p - np.concatenate([amp[0] * phi, amp[1] * phi])).max() / (np.abs(amp).max() * np.abs(phi).max())
    print(f"closed form with a sine source {TG._id(case)} theta {theta}: {err:.2e} (bar {SRC_STEP_TOL:.1e}), amplitudes {amp}")
    assert done == N and all(i.converged for i in infos) and err <= SRC_STEP_TOL


def test_wells_conserve_mass(gpu_ctx_factory):
    """No Dirichlet sets, two wells with a constant total rate Q: 1^T M (S1 p1 + S2 p2) rises by dt Q per step.

    Derivation.  Without constrained dofs F = I and the columns of A_unel sum to zero over both fields (K 1 = 0; the transfer
    terms +-(beta/mu) M cancel between the fields), so 1^T A_unel v = 0 for every v.  Summing the rows of the step equation with
    its residual r_s, (Sigma M / dt + theta A_unel) d_s = b_s - r_s:  1^T Sigma M d_s = dt (1^T b_s - 1^T r_s), and
    1^T b_s = sum_k c_k 1^T L_k = Q, because a point load is a partition of unity and constant rates give c_k = r_k.  The rise
    therefore misses dt Q by dt |1^T r_s| <= dt sqrt(2n) ||r_s||_2 (Cauchy-Schwarz).  CG + Jacobi stops on the PRECONDITIONED norm,
    ||D^-1 r_s|| <= rtol ||D^-1 b_s|| with D the diagonal of the step operator (tests/test_transient_gpu.py, the balance identity),
    so ||r_s||_2 <= dmax ||D^-1 r_s|| <= dmax rtol ||D^-1 b_s|| <= (dmax / dmin) rtol ||b_s||_2: the miss is at most
    dt (dmax / dmin) sqrt(2n) rtol ||b_s||, which is the tolerance sqrt(2n) rtol ||b_s|| (rtol = 1e-12) wherever
    dt dmax / dmin <= 1 - the test takes dmax and dmin from the exported blocks and asserts that premise.  To it comes the rounding
    of the sums formed in NumPy: z = S1 p1 + S2 p2 (2 roundings), a row of M z (at most 9 terms), the sum over n rows -
    (n + 11) eps of 1^T |M| (|S1 p1| + |S2 p2|) per state (Higham's bound for recursive summation, first order)."""
    kind, nx, ny = o.CELL_QUAD, 5, 3
    none = (np.zeros(0, dtype=np.int64),) * 2
    ctx = _context(gpu_ctx_factory, kind, nx, ny, 0, 1, none)
    n = ctx.n
    pts = np.array([[0.37, 0.61], [0.8, 0.25]])
    ctx.sources_set(None, pts, np.array([0, 1], dtype=np.int32))
    storage, theta, dt, N = (1.0, 1.0), 0.5, 0.02, 5
    rates = np.array([1.75, -0.5])
    Q = float(rates.sum())
    cfg = TG._cfg(spar.CG_JACOBI_PARAMS)
    ctx.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, storage, theta, dt)
    p = TG._initial(o.build_mesh(2, kind, nx, ny), 2)
    done, infos, norms, traj = ctx.transient_steps(cfg, p, N, record=True, coef=np.tile(rates, (N, 1)))
    M = ctx.csr(_ffi.MAT_M)
    ones = np.ones(n)
    mass = lambda v: float(ones @ (M @ (storage[0] * v[:n] + storage[1] * v[n:])))
    ulp = lambda v: float(ones @ (abs(M) @ np.abs(storage[0] * v[:n])) + ones @ (abs(M) @ np.abs(storage[1] * v[n:])))
    assert done == N and all(i.converged for i in infos)
    D = np.concatenate([ctx.csr(_ffi.MAT_A11).diagonal(), ctx.csr(_ffi.MAT_A22).diagonal()])
    print(f"conservation: dt dmax / dmin = {dt * D.max() / D.min():.3f} (the premise: at most 1)")
    assert D.min() > 0.0 and dt * D.max() / D.min() <= 1.0
    for s in range(N):
        rise = mass(traj[s + 1]) - mass(traj[s])
        tol = 1e-12 * np.sqrt(2 * n) * norms[s, 0] + (n + 11) * T.EPS * (ulp(traj[s + 1]) + ulp(traj[s]))
        print(f"conservation step {s}: rise {rise:.15e}, dt Q {dt * Q:.15e}, |difference| {abs(rise - dt * Q):.2e} (tolerance {tol:.2e})")
        assert abs(rise - dt * Q) <= tol


# ---- rate gradients ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("run", range(len(STEP_RUNS)), ids=_rid)
def test_rate_and_parameter_gradients_match_the_restatement(gpu_ctx_factory, run, theta):
    """The backward loop over the restatement's trajectory of a run WITH sources: src_grad against G[s][k] = w_s^T F L_k, and
    terms / q0 (the parameter and initial-field gradients) at the bars of tests/test_transient_adjoint_gpu.py."""
    pr = _step_problem(run, theta)
    cfg = _solver(STEP_RUNS[run])
    ctx = _step_context(gpu_ctx_factory, STEP_RUNS[run], pr)
    ctx.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, STORAGE, theta, DT, monolithic=not cfg.picard)
    n = pr["n"]
    Gf = np.random.default_rng(90 + run).standard_normal((N_STEPS + 1, 2 * n))
    sweep = A.adjoint_sweep(pr["K"], pr["M"], CF, STORAGE, theta, DT, pr["masks"], list(pr["states"]), Gf)
    Gref, Gsum = S.source_gradients(sweep, pr["loads"], pr["masks"])
    before = ctx.rhs() + (ctx.solution().copy(),)
    terms, q0, wsum, infos, done, sg = ctx.transient_adjoint(cfg, pr["states"], g=Gf, want_src_grad=True)
    assert done == N_STEPS and all(i.converged for i in infos) and sg.shape == (N_STEPS, 4)
    eg = float((np.abs(sg - Gref) / np.maximum(Gsum, 1e-300)).max())
    et = float((np.abs(terms - sweep["terms"]) / sweep["sums"]).max())
    eq = float(np.abs(q0 - sweep["q0"]).max() / np.abs(sweep["q0"]).max())
    print(f"gradients {_rid(run)} theta {theta}: src_grad {eg:.2e} of their absolute sums (bar {SRC_GRAD_BAR:g}), terms {et:.2e}, q0 {eq:.2e} "
          f"(bar {LOOP_BAR:g})")
    assert eg <= SRC_GRAD_BAR and et <= LOOP_BAR and eq <= LOOP_BAR
    assert np.count_nonzero(np.abs(Gref).max(axis=0)) >= 2     # (at most the well on a constrained node has no gradient)
    # the loop without the rate gradients: the same bits; two calls and the device variant: the same bits
    t2, q2, w2, _, _ = ctx.transient_adjoint(cfg, pr["states"], g=Gf)
    assert np.array_equal(t2, terms) and np.array_equal(q2, q0) and np.array_equal(w2, wsum)
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (pr["states"], Gf)]
    t3, q3, w3, _, _, sg3 = ctx.transient_adjoint(cfg, dev[0], g=dev[1], want_src_grad=True)
    assert np.array_equal(sg3, sg) and np.array_equal(t3, terms) and np.array_equal(q3.cpu().numpy(), q0)
    after = ctx.rhs() + (ctx.solution().copy(),)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


# ---- the public interface ---------------------------------------------------------------------------------------------------------
def _pumping_test(on_device=False):
    """The example of INTEGRATION.md "Wells and sources": one pumping well, two observation wells."""
    import perphil_amd as pa
    from perphil_amd import fd, transient

    kind, nx, ny = o.CELL_QUAD, 8, 8
    mesh = fd.Mesh(2, kind, nx, ny, 0, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    om, K, M = T.scalar_matrices(2, kind, nx, ny)
    n = om.num_nodes
    bnd = o.boundary_nodes(om)
    bcs = [fd.DirichletBC(W.sub(0), np.ones(n)), fd.DirichletBC(W.sub(1), np.ones(n))]      # p = 1 on the whole boundary
    params = pa.DPPParameters(k1=CF.k1, k2=CF.k2, beta=CF.beta, mu=CF.mu)
    N, dt, theta, storage = 6, 0.05, 1.0, (0.3, 5.0)
    schedule = np.array([0.0, -2.0, -2.0, -2.0, 0.0, 0.0, 0.0])              # pump for three steps, then recover
    well = transient.Well([0.5, 0.5], schedule, network=0)
    recharge = transient.DistributedSource(lambda X: np.sin(np.pi * X[:, 0]) * X[:, 1], rate=lambda t: 0.5 + t, network=1)
    obs = np.array([[0.25, 0.5], [0.8, 0.7]])
    sp_ = {**spar.CG_JACOBI_PARAMS, "ksp_rtol": 1e-12, "ksp_atol": 1e-300}
    return dict(pa=pa, fd=fd, transient=transient, W=W, V=V, om=om, K=K, M=M, n=n, bnd=bnd, bcs=bcs, params=params, N=N, dt=dt, theta=theta,
                storage=storage, sources=[well, recharge], obs=obs, sp=sp_, schedule=schedule,
                kw=dict(storage=storage, theta=theta, solver_parameters=sp_, on_device=on_device))


@pytest.mark.parametrize("on_device", [False, True])
def test_pumping_test_example(on_device):
    q = _pumping_test(on_device)
    pa, n, N, dt = q["pa"], q["n"], q["N"], q["dt"]
    p0 = np.ones(2 * n)
    ts = pa.solve_dpp_transient(q["W"], q["params"], q["bcs"], p0, dt, N, observe_at=q["obs"], sources=q["sources"], **q["kw"])
    resident = ts.solution.on_device                   # (asked before vector() brings the values to the host)
    # the restatement: M f from the oracle's M, the well from the oracle's shape functions
    X = q["om"].coords
    f = np.sin(np.pi * X[:, 0]) * X[:, 1]
    loads = np.concatenate([S.point_loads(o.CELL_QUAD, 1, 8, 8, 0, [[0.5, 0.5]], [0], q["om"])[0], S.mass_load(q["M"], f, 1)[None]])
    rates = np.stack([q["schedule"], 0.5 + dt * np.arange(N + 1)], axis=1)
    masks = T.masks_of(n, q["bnd"], q["bnd"])
    g = (np.where(masks[0], 1.0, 0.0), np.where(masks[1], 1.0, 0.0))
    states, bn, dn = S.theta_steps(q["K"], q["M"], CF, q["storage"], q["theta"], dt, masks, g, p0, N, loads, S.coefficients(rates, q["theta"]))
    err = np.abs(ts.solution.vector() - states[-1]).max() / np.abs(states[-1]).max()
    E, _ = A.point_matrix(o.CELL_QUAD, 1, 8, 8, 0, q["obs"])
    obs_ref = np.stack([np.stack([E @ st[:n], E @ st[n:]], axis=1) for st in states])
    eo = np.abs(ts.observations - obs_ref).max() / np.abs(obs_ref).max()
    print(f"pumping test on_device={on_device}: final state {err:.2e}, observations {eo:.2e} (bar {SRC_STEP_TOL:.1e}); drawdown at the "
          f"observation wells {1.0 - ts.observations[:, :, 0].min(axis=0)}")
    assert ts.steps_done == N and resident == on_device and np.array_equal(ts.source_rates, rates)
    assert err <= SRC_STEP_TOL and eo <= SRC_STEP_TOL
    assert np.allclose(ts.rhs_norms, bn, rtol=1e-8, atol=0) and np.allclose(ts.increment_norms, dn, rtol=1e-8, atol=0)
    assert ts.observations[3, 0, 0] < 1.0 - 1e-3                                    # the pumping shows at the observation well
    # whatever the chunking (1 step with observe_at, 2 with record_every, 4 + 2, the whole run): the same bits
    two = pa.solve_dpp_transient(q["W"], q["params"], q["bcs"], p0, dt, N, record_every=2, sources=q["sources"], **q["kw"])
    four = pa.solve_dpp_transient(q["W"], q["params"], q["bcs"], p0, dt, N, record_every=4, sources=q["sources"], **q["kw"])
    whole = pa.solve_dpp_transient(q["W"], q["params"], q["bcs"], p0, dt, N, sources=q["sources"], record_trajectory=True, **q["kw"])
    traj = whole.trajectory.cpu().numpy() if torch.is_tensor(whole.trajectory) else whole.trajectory
    for other in (two, four, whole):
        assert np.array_equal(other.solution.vector(), ts.solution.vector()) and np.array_equal(other.rhs_norms, ts.rhs_norms)
    assert sorted(two.snapshots) == [0, 2, 4, 6] and sorted(four.snapshots) == [0, 4, 6]
    for step, fn in list(two.snapshots.items()) + list(four.snapshots.items()):
        assert np.array_equal(fn.vector(), traj[step]), step
        for fld in (0, 1):
            assert np.array_equal(np.asarray(fn.sub(fld).at(q["obs"])).reshape(-1), ts.observations[step, :, fld])
    # no sources and an empty list: today's calls, the same bits
    a = pa.solve_dpp_transient(q["W"], q["params"], q["bcs"], p0, dt, N, **q["kw"])
    b = pa.solve_dpp_transient(q["W"], q["params"], q["bcs"], p0, dt, N, sources=[], **q["kw"])
    assert a.source_rates is None and b.source_rates is None and np.array_equal(a.solution.vector(), b.solution.vector())
    assert np.abs(a.solution.vector() - ts.solution.vector()).max() > 1e-3


def test_rate_gradient_against_a_central_difference():
    """dJ/dr_k(t_j) of transient_sensitivities(wrt_sources=True) for the pumping well at j = 2 against a central difference
    through solve_dpp_transient, chosen as tests/test_transient_adjoint_host.py chooses: relative step 1e-6, bar 1e-5 relative."""
    q = _pumping_test(True)
    pa, transient, N, dt, n = q["pa"], q["transient"], q["N"], q["dt"], q["n"]
    p0 = np.ones(2 * n)
    data = np.random.default_rng(4).standard_normal((N + 1, 2, 2))
    kw = dict(q["kw"])

    def J(schedule):
        src = [transient.Well([0.5, 0.5], schedule, network=0), q["sources"][1]]
        ts = pa.solve_dpp_transient(q["W"], q["params"], q["bcs"], p0, dt, N, observe_at=q["obs"], sources=src, **kw)
        return float((ts.observations * data).sum())

    ts = pa.solve_dpp_transient(q["W"], q["params"], q["bcs"], p0, dt, N, sources=q["sources"], record_trajectory=True, **kw)
    s = transient.transient_sensitivities(q["W"], q["params"], q["bcs"], ts, dJ_dobs=data, observe_at=q["obs"], storage=q["storage"],
                                          theta=q["theta"], dt=dt, solver_parameters=q["sp"], sources=q["sources"], wrt_sources=True)
    assert s.source_rates.shape == (N + 1, 2)
    j = 2
    h = 1e-6 * abs(q["schedule"][j])
    e = np.zeros(N + 1)
    e[j] = h
    fd = (J(q["schedule"] + e) - J(q["schedule"] - e)) / (2.0 * h)
    rel = abs(fd - s.source_rates[j, 0]) / abs(fd)
    print(f"dJ/dr_0(t_{j}): adjoint {s.source_rates[j, 0]:.9e}, central difference {fd:.9e}, relative {rel:.2e} (bar 1e-5)")
    assert rel <= 1e-5
    # the other gradients do not change with wrt_sources
    s0 = transient.transient_sensitivities(q["W"], q["params"], q["bcs"], ts, dJ_dobs=data, observe_at=q["obs"], storage=q["storage"],
                                           theta=q["theta"], dt=dt, solver_parameters=q["sp"])
    assert s0.source_rates is None and np.array_equal(s0.terms, s.terms) and (s0.k1, s0.mu) == (s.k1, s.mu)


def test_backward_through_a_run_with_wells():
    q = _pumping_test(True)
    transient, N, dt, n = q["transient"], q["N"], q["dt"], q["n"]
    p0 = np.ones(2 * n)
    rate = torch.tensor(q["schedule"], dtype=torch.float64, requires_grad=True)                   # (a host tensor: its gradient stays there)
    level = torch.tensor(0.5, dtype=torch.float64, device="cuda", requires_grad=True)
    src = [transient.Well([0.5, 0.5], rate, network=0), transient.DistributedSource(np.ones(n), level, network=1)]
    data = torch.from_numpy(np.random.default_rng(4).standard_normal((N + 1, 2, 2))).cuda()
    k1 = torch.tensor(CF.k1, dtype=torch.float64, requires_grad=True)
    obs = transient.solve_dpp_transient_torch(q["W"], k1, CF.k2, CF.beta, CF.mu, q["storage"][0], q["storage"][1], q["bcs"], p0, dt, N,
                                              q["theta"], q["sp"], observe_at=q["obs"], sources=src)
    loss = 0.5 * torch.sum((obs - data) ** 2)
    loss.backward()
    plain = [transient.Well([0.5, 0.5], q["schedule"], network=0), transient.DistributedSource(np.ones(n), 0.5, network=1)]
    ts = q["pa"].solve_dpp_transient(q["W"], q["params"], q["bcs"], p0, dt, N, sources=plain, record_trajectory=True, **q["kw"])
    s = transient.transient_sensitivities(q["W"], q["params"], q["bcs"], ts, dJ_dobs=(obs.detach() - data), observe_at=q["obs"],
                                          storage=q["storage"], theta=q["theta"], dt=dt, solver_parameters=q["sp"], sources=plain,
                                          wrt_sources=True)
    print(f"autograd: rate.grad {rate.grad.numpy()}, level.grad {float(level.grad):.6e}, k1.grad {float(k1.grad):.6e}")
    assert not rate.grad.is_cuda and np.array_equal(rate.grad.numpy(), s.source_rates[:, 0])
    assert level.grad.is_cuda and float(level.grad) == float(s.source_rates[:, 1].sum()) and float(k1.grad) == s.k1
    assert np.abs(s.source_rates[:, 0]).max() > 0.0


# ---- refusals through the C ABI -----------------------------------------------------------------------------------------------------
def test_source_refusals_leave_the_context_usable(gpu_ctx_factory):
    kind, nx, ny = o.CELL_QUAD, 4, 4
    om = o.build_mesh(2, kind, nx, ny)
    n = om.num_nodes
    bnd = o.boundary_nodes(om)
    lib = _ffi.lib
    ctx = gpu_ctx_factory()
    nout, cnt, done = C.c_int64(), C.c_int64(), C.c_int(0)
    x = np.array([[0.5, 0.5], [0.1, 0.9]])
    fld = np.array([0, 1], dtype=np.int32)
    dense = np.ones((1, 2 * n))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    err = lambda: lib.pph_last_error(ctx._h)
    assert lib.pph_sources_set(ctx._h, None, 0, ptr(x), ptr(fld), 2, 1e-12, C.byref(nout)) == _ffi.PPH_ERR_INVALID
    assert b"before pph_mesh_build" in err()
    ctx.mesh_build(2, kind, nx, ny)
    for f in (0, 1):
        ctx.set_dirichlet(f, bnd, np.zeros(len(bnd)))
    for args, msg in [((None, 1, ptr(x), ptr(fld), 2, 1e-12, C.byref(nout)), b"NULL buffer"),
                      ((ptr(dense), 1, None, ptr(fld), 2, 1e-12, C.byref(nout)), b"NULL buffer"),
                      ((ptr(dense), 1, ptr(x), None, 2, 1e-12, C.byref(nout)), b"NULL buffer"),
                      ((ptr(dense), 1, ptr(x), ptr(fld), 2, 1e-12, None), b"NULL buffer"),
                      ((ptr(dense), -1, ptr(x), ptr(fld), 2, 1e-12, C.byref(nout)), b"negative count"),
                      ((ptr(dense), 1, ptr(x), ptr(np.array([0, 2], dtype=np.int32)), 2, 1e-12, C.byref(nout)), b"networks are 0 and 1"),
                      ((ptr(dense), 1, ptr(x), ptr(fld), 2, 0.5, C.byref(nout)), b"tol must be")]:
        assert lib.pph_sources_set(ctx._h, *args) == _ffi.PPH_ERR_INVALID
        assert msg in err(), err()
    assert lib.pph_sources_count(ctx._h, C.byref(cnt)) == 0 and cnt.value == -1
    b = np.zeros(2 * n)
    assert lib.pph_sources_apply(ctx._h, ptr(np.ones(3)), ptr(b)) == _ffi.PPH_ERR_INVALID and b"no source set" in err()
    cfg = TG._cfg(spar.CG_JACOBI_PARAMS)
    ctx.transient_begin(1.0, 0.5, 2.0, 1.0, (1.0, 2.0), 1.0, 0.1)
    p = np.ones(2 * n)
    coef = np.ones((2, 3))
    assert lib.pph_transient_steps_sources(ctx._h, C.byref(cfg), ptr(p), 2, 0.0, None, None, C.byref(done), None, ptr(coef), 3) == _ffi.PPH_ERR_INVALID
    assert b"no source set" in err()
    assert ctx.sources_set(dense, x, fld) == 0
    # a refused set leaves the set as it was
    assert lib.pph_sources_set(ctx._h, ptr(dense), 1, ptr(x), ptr(np.array([0, 5], dtype=np.int32)), 2, 1e-12, C.byref(nout)) == _ffi.PPH_ERR_INVALID
    assert ctx.sources_count() == 3
    assert lib.pph_sources_apply(ctx._h, None, ptr(b)) == _ffi.PPH_ERR_INVALID and b"NULL buffer" in err()
    assert lib.pph_sources_apply(ctx._h, ptr(np.ones(3)), None) == _ffi.PPH_ERR_INVALID and b"NULL buffer" in err()
    assert lib.pph_transient_steps_sources(ctx._h, C.byref(cfg), ptr(p), 2, 0.0, None, None, C.byref(done), None, ptr(coef), 2) == _ffi.PPH_ERR_INVALID
    assert b"coef has 2 columns" in err()
    assert lib.pph_transient_steps_sources(ctx._h, C.byref(cfg), ptr(p), 2, 0.0, None, None, C.byref(done), None, None, 3) == _ffi.PPH_ERR_INVALID
    assert b"NULL buffer" in err()
    with pytest.raises(ValueError, match="coef must have shape"):
        ctx.transient_steps(cfg, p, 2, coef=np.ones((3, 3)))
    traj = np.ones((3, 2 * n))
    terms, q0 = np.zeros((2, 5)), np.zeros(2 * n)
    sg = np.zeros((2, 2))
    call = lambda sgp, K: lib.pph_transient_adjoint_sources(ctx._h, C.byref(cfg), ptr(traj), ptr(traj), None, 0, None, 1e-12, 2, ptr(terms),
                                                            ptr(q0), None, None, C.byref(done), sgp, K)
    assert call(ptr(sg), 2) == _ffi.PPH_ERR_INVALID and b"src_grad has 2 columns" in err()
    assert call(None, 3) == _ffi.PPH_ERR_INVALID and b"NULL buffer" in err()
    ctx.sources_clear()
    assert call(ptr(sg), 3) == _ffi.PPH_ERR_INVALID and b"no source set" in err()
    with pytest.raises(ValueError, match="no source set"):
        ctx.transient_adjoint(cfg, traj, g=traj, want_src_grad=True)
    # ... and still works
    assert ctx.sources_set(dense, x, fld) == 0
    d, infos, norms = ctx.transient_steps(cfg, p, 2, coef=coef)
    assert d == 2 and all(i.converged for i in infos) and np.all(np.isfinite(p)) and np.abs(p - 1.0).max() > 1e-3
    out = ctx.transient_adjoint(cfg, traj, g=traj, want_src_grad=True)
    assert out[4] == 2 and out[5].shape == (2, 3) and np.all(np.isfinite(out[5]))
