"""The transient adjoint on the device (perphil_amd/csrc/pph_transient_adjoint.hip, the recording variant of the step loop in
pph_transient.hip, perphil_amd/transient.py) against the restatement of tests/transient_adjoint_reference.py.

Bars.  The bilinear kernel alone: every form within 1e3 eps of its absolute sum (|w1|^T |K| |pm1| ...), the bar of
test_transient_gpu.py.  The transposed evaluation: <c, u.at(x)> = <E^T c, u> to 1e3 eps of sum |c_m| |phi_a(x_m)| |u_a|.  The loop:
the larger of 1e-10 and 10 x what the restatement itself loses when its solves run by the oracle's pcg at rtol 1e-13 instead of
splu - measured on the CPU over the runs of this file: at most 7.4e-13 (terms, of their absolute sums), 1.4e-13 (q0) and 3.6e-14
(boundary gradient), of their largest entries (tests/README_transient_adjoint.md); 10 x that is below 1e-10, so the bar is 1e-10.
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

pytestmark = pytest.mark.gpu

CF, BAR = TG.CF, TG.BAR
LOOP_BAR = 1e-10
PASS_BOXES = 2048 * 256      # boxes one pass of k_transient_bilinear's grid covers


def _spread(rng, size):
    """Random values with magnitudes spread over four decades."""
    return rng.standard_normal(size) * 10.0 ** rng.uniform(-2, 2, size)


def _mesh_context(make, kind, nx, ny, nz, degree):
    ctx = make()
    if degree == 1:
        ctx.mesh_build(TG._dim(kind), kind, nx, ny, nz)
    else:
        ctx.mesh_build_lagrange(TG._dim(kind), kind, nx, ny, nz, degree)
    return ctx


def _check_forms(tag, got, ref, sums):
    ratio = np.abs(np.asarray(got) - ref) / sums / T.EPS
    print(f"{tag}: |form - restatement| / (eps absolute sum) = {np.array2string(ratio, precision=2)} (bar 1e3)")
    assert np.all(np.abs(np.asarray(got) - ref) <= BAR * sums)


# ---- the kernel alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("case", TG.SMALL, ids=TG._id)
def test_bilinear_forms_on_small_shapes(gpu_ctx_factory, case, degree, theta):
    kind, nx, ny, nz = case
    ctx = _mesh_context(gpu_ctx_factory, kind, nx, ny, nz, degree)
    if degree == 1:
        _, K, M = T.scalar_matrices(TG._dim(kind), kind, nx, ny, nz)
    else:
        K, M = ctx.csr(_ffi.MAT_K), ctx.csr(_ffi.MAT_M)
    n = ctx.n
    assert K.shape == (n, n)
    rng = np.random.default_rng(300 + TG.SMALL.index(case) + 50 * degree)
    w, p0, p1 = (_spread(rng, 2 * n) for _ in range(3))
    ref, sums = A.step_forms(K, M, w, p0, p1, theta)
    got = ctx.transient_bilinear(w, p0, p1, theta)
    _check_forms(f"{TG._id(case)} degree {degree} theta {theta}", got, ref, sums)
    assert got == ctx.transient_bilinear(w, p0, p1, theta)
    dev = ctx.transient_bilinear(*(torch.from_numpy(v.copy()).cuda() for v in (w, p0, p1)), theta)
    assert dev == got


LARGE = [(o.CELL_QUAD, 1, 1024, 1024, 0), (o.CELL_TRI, 1, 1024, 1024, 0), (o.CELL_HEX, 1, 128, 64, 128), (o.CELL_TET, 1, 128, 64, 128),
         (o.CELL_QUAD, 2, 1024, 1024, 0)]


@pytest.mark.parametrize("case", LARGE, ids=lambda c: f"{TG.NAMES[c[0]]}{c[2]}x{c[3]}x{c[4]}-deg{c[1]}")
def test_bilinear_forms_past_one_pass_of_the_grid(gpu_ctx_factory, case):
    """1 048 576 boxes: the 2048 x 256 grid makes a second pass.  Powers of two, for the reason
    test_transient_gpu.test_more_nodes_than_one_pass_of_the_grid gives (the exported K is integrated on stored coordinates).
    Degree 1: the reference comes from the context's exported K and M; degree 2 (quadrilaterals): from the matrix-free products
    of tests/p2_matfree.py.  Second run: w supported only on nodes of boxes >= 524 288 - the second pass carries the whole value."""
    kind, degree, nx, ny, nz = case
    ctx = _mesh_context(gpu_ctx_factory, kind, nx, ny, nz, degree)
    n = ctx.n
    cells = ctx.dofmap()
    cpb = cells.shape[0] // (nx * ny * max(nz, 1))
    assert cells.shape[0] // cpb == 2 * PASS_BOXES
    rng = np.random.default_rng(77 + kind + degree)
    p0, p1 = rng.standard_normal(2 * n), rng.standard_normal(2 * n)
    if degree == 1:
        parts = A.csr_products(ctx.csr(_ffi.MAT_K), ctx.csr(_ffi.MAT_M))
    else:
        import p2_matfree as P2

        parts = P2.Operator(kind, nx, ny, nz).parts
    theta = 0.5
    prod = A.step_products(parts, p0, p1, theta)
    late = np.unique(cells[PASS_BOXES * cpb:])
    w_all = rng.standard_normal(2 * n)
    w_late = np.zeros(2 * n)
    w_late[late] = rng.standard_normal(late.size)
    w_late[n + late] = rng.standard_normal(late.size)
    for tag, w in (("random w", w_all), ("w on the second pass", w_late)):
        ref, sums = A.forms_of(w, prod)
        got = ctx.transient_bilinear(w, p0, p1, theta)
        _check_forms(f"{TG.NAMES[kind]} degree {degree} {tag}", got, ref, sums)
        assert all(v != 0.0 for v in got)
        assert got == ctx.transient_bilinear(w, p0, p1, theta)


# ---- transposed point evaluation --------------------------------------------------------------------------------------------
EVAL_CASES = [(o.CELL_QUAD, 5, 3, 0), (o.CELL_TRI, 4, 3, 0), (o.CELL_HEX, 3, 4, 2), (o.CELL_TET, 3, 2, 3)]


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("case", EVAL_CASES, ids=TG._id)
def test_transposed_evaluation(gpu_ctx_factory, case, degree):
    kind, nx, ny, nz = case
    dim = TG._dim(kind)
    ctx = _mesh_context(gpu_ctx_factory, kind, nx, ny, nz, degree)
    n = ctx.n
    rng = np.random.default_rng(PE.case_seed(kind, degree))
    rnd = PE.random_points(kind, degree, 200)
    outside_pts = np.array([[1.5] * dim, [-0.2] + [0.5] * (dim - 1), [0.5] * (dim - 1) + [1.0 + 1e-6]])
    pts = np.ascontiguousarray(np.concatenate([rnd, rnd[:20], rnd[5:6].repeat(4, axis=0), PE.deliberate_points(kind, nx, ny, nz),
                                               outside_pts]))
    m = len(pts)
    u, c = _spread(rng, n), _spread(rng, m)
    val, _, nout = ctx.eval_points(u, pts)
    inside = ~np.isnan(val[:, 0])
    assert nout == 3 == int((~inside).sum()) and not inside[-3:].any()
    b, nout_t = ctx.eval_points_adjoint(pts, c)
    assert nout_t == 3
    E, _ = A.point_matrix(kind, degree, nx, ny, nz, pts)
    scale = float(abs(c) @ (abs(E) @ abs(u)))
    lhs, rhs = float(c[inside] @ val[inside, 0]), float(b @ u)
    print(f"{TG._id(case)} degree {degree}: <c, E u> - <E^T c, u> = {lhs - rhs:.2e}, {abs(lhs - rhs) / scale / T.EPS:.2f} eps of sum |terms| "
          f"(bar 1e3), {m} points")
    assert abs(lhs - rhs) <= BAR * scale
    # outside points contribute nothing: the same result without them; duplicates add up: weights 1 at one point k times
    b_in, _ = ctx.eval_points_adjoint(pts[:-3], c[:-3])
    assert np.array_equal(b, b_in)
    one, _ = ctx.eval_points_adjoint(rnd[5:6], np.ones(1))
    five, _ = ctx.eval_points_adjoint(rnd[5:6].repeat(5, axis=0), np.ones(5))
    assert np.allclose(five, 5.0 * one, rtol=4 * T.EPS, atol=0)
    assert abs(one.sum() - 1.0) <= 64 * T.EPS      # (partition of unity: at most 27 basis values of magnitude <= 1)
    # two calls, the device variant, and accumulation into a caller's array: the same bits
    assert np.array_equal(b, ctx.eval_points_adjoint(pts, c)[0])
    bd, nd = ctx.eval_points_adjoint(torch.from_numpy(pts).cuda(), torch.from_numpy(c).cuda())
    assert bd.is_cuda and nd == 3 and np.array_equal(bd.cpu().numpy(), b)
    acc = np.ones(n)
    ctx.eval_points_adjoint(pts, c, out=acc)
    assert np.allclose(acc - 1.0, b, rtol=0, atol=4 * T.EPS * (1.0 + abs(b).max()))
    # two components at once: each the scalar result
    c2 = np.stack([c, -2.0 * c], axis=1)
    b2, _ = ctx.eval_points_adjoint(pts, c2, ncomp=2)
    assert np.array_equal(b2.reshape(n, 2)[:, 0], b) and np.array_equal(b2.reshape(n, 2)[:, 1], -2.0 * b)


# ---- recording ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [TG.STEP_RUNS[0], TG.STEP_RUNS[2]], ids=lambda r: f"{TG._id(r[0])}-{r[2]}")
def test_recorded_rows_are_the_states_of_plain_steps(gpu_ctx_factory, run):
    (kind, nx, ny, nz), degree, name = run
    om, K, M = T.scalar_matrices(TG._dim(kind), kind, nx, ny, nz)
    n = om.num_nodes
    nodes = TG._dirichlet_sets(kind, nx, ny, nz, "mixed")
    g = TG._dirichlet_data(n, nodes, 6)
    cfg = TG._cfg(*TG.SOLVERS[name])
    ctx = TG._shifted_context(gpu_ctx_factory, kind, nx, ny, nz, nodes, g)
    p0 = TG._initial(om, 2)
    storage, theta, dt, N = (0.3, 5.0), 0.5, 0.02, 4
    ctx.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, storage, theta, dt)
    plain = p0.copy()
    d0, _, norms0 = ctx.transient_steps(cfg, plain, N)
    before = ctx.rhs() + (ctx.solution().copy(),)
    rec = p0.copy()
    d1, infos, norms1, traj = ctx.transient_steps(cfg, rec, N, record=True)
    after = ctx.rhs() + (ctx.solution().copy(),)
    assert d0 == d1 == N and traj.shape == (N + 1, 2 * n)
    assert np.array_equal(rec, plain) and np.array_equal(norms0, norms1)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    con = np.concatenate(T.masks_of(n, *nodes))
    assert np.array_equal(traj[0], np.where(con, np.concatenate(g), p0))
    for s in range(1, N + 1):
        q = p0.copy()
        ctx.transient_steps(cfg, q, s)
        assert np.array_equal(traj[s], q), s
    td = torch.from_numpy(p0.copy()).cuda()      # the device variant: the same bits
    d2, _, norms2, trajd = ctx.transient_steps(cfg, td, N, record=True)
    assert d2 == N and trajd.is_cuda and np.array_equal(trajd.cpu().numpy(), traj) and np.array_equal(norms2, norms0)


# ---- the loop against the restatement -------------------------------------------------------------------------------------------
N_LOOP = 6
WELLS = 7


@functools.lru_cache(maxsize=None)
def _loop_problem(run_index, theta):
    """Matrices, sets, data, the restatement's states and functional derivatives of a run, computed once."""
    (kind, nx, ny, nz), degree, name = TG.STEP_RUNS[run_index]
    if degree == 1:
        om, K, M = T.scalar_matrices(TG._dim(kind), kind, nx, ny, nz)
        n = om.num_nodes
        nodes = TG._dirichlet_sets(kind, nx, ny, nz, "mixed")
        p0 = TG._initial(om, 2)
    else:
        probe = _ffi.Context(0)
        probe.mesh_build_lagrange(TG._dim(kind), kind, nx, ny, nz, degree)
        n = probe.n
        K, M = probe.csr(_ffi.MAT_K), probe.csr(_ffi.MAT_M)
        probe.close()
        rng = np.random.default_rng(12)
        nodes = (np.sort(rng.choice(n, n // 5, replace=False)), np.sort(rng.choice(n, n // 6, replace=False)))
        p0 = rng.standard_normal(2 * n)
    masks = T.masks_of(n, *nodes)
    g = TG._dirichlet_data(n, nodes, 6)
    storage, dt = (0.3, 5.0), 0.02
    states, _, _ = T.theta_steps(K, M, CF, storage, theta, dt, masks, g, p0, N_LOOP)
    rng = np.random.default_rng(90 + run_index)
    G = rng.standard_normal((N_LOOP + 1, 2 * n))
    pts = np.ascontiguousarray(rng.random((WELLS, TG._dim(kind))))
    pts[0] = 0.5                                                  # (a well on a node / a face of most meshes)
    oc = rng.standard_normal((N_LOOP + 1, WELLS, 2))
    E, outside = A.point_matrix(kind, degree, nx, ny, nz, pts)
    assert not outside.any()
    G_obs = np.stack([np.concatenate([E.T @ oc[s, :, 0], E.T @ oc[s, :, 1]]) for s in range(N_LOOP + 1)])
    return dict(K=K, M=M, n=n, nodes=nodes, masks=masks, g=g, storage=storage, dt=dt, states=np.stack(states), G=G, pts=pts, oc=oc,
                G_obs=G_obs)


def _compare_loop(tag, pr, ctx, theta, G_ref, terms, q0, wsum):
    K, M, masks = pr["K"], pr["M"], pr["masks"]
    con = np.concatenate(masks)
    sweep = A.adjoint_sweep(K, M, CF, pr["storage"], theta, pr["dt"], masks, list(pr["states"]), G_ref)
    ref = A.gradients(K, M, CF, pr["storage"], pr["dt"], masks, G_ref, sweep)
    et = float((np.abs(terms - sweep["terms"]) / sweep["sums"]).max())
    eq = float(np.abs(q0 - sweep["q0"]).max() / np.abs(sweep["q0"]).max())
    bc = np.where(con, G_ref.sum(axis=0) - ctx.dpp_nodal_flux(wsum, CF.k1, CF.k2, CF.beta, CF.mu), 0.0)
    eb = float(np.abs(bc - ref["bc"]).max() / np.abs(ref["bc"]).max())
    print(f"{tag}: terms {et:.2e} of their absolute sums, q0 {eq:.2e}, boundary gradient {eb:.2e} of the largest entry (bar {LOOP_BAR:g})")
    assert et <= LOOP_BAR and eq <= LOOP_BAR and eb <= LOOP_BAR
    assert np.all(q0[con] == 0.0) and np.all(wsum[con] == 0.0)


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("run", range(len(TG.STEP_RUNS)),
                         ids=lambda i: f"{TG._id(TG.STEP_RUNS[i][0])}-deg{TG.STEP_RUNS[i][1]}-{TG.STEP_RUNS[i][2]}")
def test_backward_loop_matches_the_restatement(gpu_ctx_factory, run, theta):
    """Dense G, and separately the observation form with 7 wells; the trajectory is the restatement's, so that the comparison is
    about the backward loop.  All solves at rtol 1e-12."""
    (kind, nx, ny, nz), degree, name = TG.STEP_RUNS[run]
    pr = _loop_problem(run, theta)
    params, nonlinear = (spar.FIELDSPLIT_PMG_PARAMS, False) if degree == 2 else TG.SOLVERS[name]
    cfg = TG._cfg(params, nonlinear)
    ctx = TG._shifted_context(gpu_ctx_factory, kind, nx, ny, nz, pr["nodes"], pr["g"], degree)
    ctx.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, pr["storage"], theta, pr["dt"], monolithic=not cfg.picard)
    before = ctx.rhs() + (ctx.solution().copy(),)
    tag = f"{TG._id((kind, nx, ny, nz))} degree {degree} {name} theta {theta}"
    terms, q0, wsum, infos, done = ctx.transient_adjoint(cfg, pr["states"], g=pr["G"])
    assert done == N_LOOP and all(i.converged for i in infos) and terms.shape == (N_LOOP, 5)
    _compare_loop(tag + " dense G", pr, ctx, theta, pr["G"], terms, q0, wsum)
    t2, q2, w2, _, _ = ctx.transient_adjoint(cfg, pr["states"], g=pr["G"])
    assert np.array_equal(t2, terms) and np.array_equal(q2, q0) and np.array_equal(w2, wsum)
    after = ctx.rhs() + (ctx.solution().copy(),)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    # the observation form, on device tensors: the same loop fed through the transposed evaluation
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (pr["states"], pr["pts"], pr["oc"])]
    t3, q3, w3, infos, done = ctx.transient_adjoint(cfg, dev[0], obs_x=dev[1], obs_c=dev[2])
    assert done == N_LOOP and all(i.converged for i in infos) and q3.is_cuda and w3.is_cuda
    _compare_loop(tag + " wells", pr, ctx, theta, pr["G_obs"], t3, q3.cpu().numpy(), w3.cpu().numpy())
    t4, q4, w4, _, _ = ctx.transient_adjoint(cfg, pr["states"], obs_x=pr["pts"], obs_c=pr["oc"])      # host variant: the same bits
    assert np.array_equal(t4, t3) and np.array_equal(q4, q3.cpu().numpy()) and np.array_equal(w4, w3.cpu().numpy())
    # both at once add up: G + E^T c
    t5, q5, _, _, _ = ctx.transient_adjoint(cfg, pr["states"], g=pr["G"], obs_x=pr["pts"], obs_c=pr["oc"], want_wsum=False)
    assert np.abs(q5 - (q0 + q4)).max() <= 1e-9 * np.abs(q0).max()
    after = ctx.rhs() + (ctx.solution().copy(),)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_zero_functional_takes_no_solve(gpu_ctx_factory):
    """q = 0 gives w = 0 without entering a Krylov loop: a functional of the constrained dofs alone."""
    pr = _loop_problem(0, 1.0)
    (kind, nx, ny, nz), _, name = TG.STEP_RUNS[0]
    cfg = TG._cfg(*TG.SOLVERS[name])
    ctx = TG._shifted_context(gpu_ctx_factory, kind, nx, ny, nz, pr["nodes"], pr["g"])
    ctx.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, pr["storage"], 1.0, pr["dt"])
    con = np.concatenate(pr["masks"])
    G = np.where(con, 3.0, 0.0)[None].repeat(N_LOOP + 1, axis=0)
    terms, q0, wsum, infos, done = ctx.transient_adjoint(cfg, pr["states"], g=G)
    assert done == N_LOOP and all(i.iterations == 0 and i.converged for i in infos)
    assert np.all(terms == 0.0) and np.all(q0 == 0.0) and np.all(wsum == 0.0)


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def _public_problem():
    import perphil_amd as pa
    from perphil_amd import fd

    kind, nx, ny = o.CELL_QUAD, 6, 5
    om, K, M = T.scalar_matrices(2, kind, nx, ny)
    n = om.num_nodes
    b = o.boundary_nodes(om)
    masks = T.masks_of(n, b, b)
    g = (np.where(masks[0], 1.0 + om.coords[:, 0], 0.0), np.where(masks[1], 0.5 - om.coords[:, 1], 0.0))
    mesh = fd.Mesh(2, kind, nx, ny, 0, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    bcs = [fd.DirichletBC(W.sub(0), g[0].copy()), fd.DirichletBC(W.sub(1), g[1].copy())]
    params = pa.DPPParameters(k1=CF.k1, k2=CF.k2, beta=CF.beta, mu=CF.mu)
    p0 = np.concatenate([np.cos(2.0 * om.coords[:, 0]) + om.coords[:, 1], 0.3 + 0.5 * np.sin(3.0 * om.coords[:, 1])])
    pts = np.array([[0.5, 0.5], [0.21, 0.77], [0.9, 0.05], [0.0, 1.0], [0.33, 0.33], [0.61, 0.2], [0.75, 0.75]])
    sp_ = {**spar.CG_JACOBI_PARAMS, "ksp_rtol": 1e-12, "ksp_atol": 1e-300}
    return dict(om=om, K=K, M=M, n=n, masks=masks, g=g, mesh=mesh, V=V, W=W, bcs=bcs, params=params, p0=p0, pts=pts, sp=sp_,
                storage=(0.3, 5.0), theta=0.5, dt=0.02, N=5)


def test_transient_sensitivities_are_the_loops_numbers():
    import perphil_amd as pa
    from perphil_amd import fd, transient

    q = _public_problem()
    W, N, n = q["W"], q["N"], q["n"]
    fw = dict(storage=q["storage"], theta=q["theta"], solver_parameters=q["sp"])
    kw = dict(fw, dt=q["dt"])
    ts = pa.solve_dpp_transient(W, q["params"], q["bcs"], q["p0"], q["dt"], N, observe_at=q["pts"], on_device=True,
                                record_trajectory=True, **fw)
    plain = pa.solve_dpp_transient(W, q["params"], q["bcs"], q["p0"], q["dt"], N, observe_at=q["pts"], on_device=True, **fw)
    traj = ts.trajectory
    assert traj.is_cuda and tuple(traj.shape) == (N + 1, 2 * n) and plain.trajectory is None
    assert np.array_equal(ts.solution.vector(), plain.solution.vector()) and np.array_equal(ts.observations, plain.observations)
    assert np.array_equal(traj[-1].cpu().numpy(), ts.solution.vector())
    states, _, _ = T.theta_steps(q["K"], q["M"], CF, q["storage"], q["theta"], q["dt"], q["masks"], q["g"], q["p0"], N)
    assert abs(traj.cpu().numpy() - np.stack(states)).max() <= TG.STEP_TOL * abs(states[-1]).max()
    rng = np.random.default_rng(8)
    dJ = torch.from_numpy(rng.standard_normal((N + 1, len(q["pts"]), 2))).cuda()
    before = dict(_ffi.fetch_stats)
    s = transient.transient_sensitivities(W, q["params"], q["bcs"], ts, dJ_dobs=dJ, observe_at=q["pts"], wrt_bcs=True, **kw)
    assert _ffi.fetch_stats == before and s.initial.on_device and all(f.on_device for f in s.bcs)
    assert isinstance(s, transient.TransientSensitivities) and s.info["converged"] and s.terms.shape == (N, 5)
    # the C loop on the same numbers
    ctx = q["mesh"].context()
    cfg, _ = pa.solver.translate_options(q["sp"])
    ctx.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, q["storage"], q["theta"], q["dt"])
    terms, q0, wsum, _, _ = ctx.transient_adjoint(cfg, traj, obs_x=torch.from_numpy(q["pts"]).cuda(), obs_c=dJ)
    assert np.array_equal(terms, s.terms) and np.array_equal(q0.cpu().numpy(), s.initial.vector())
    tot = np.zeros(5)
    for k in range(N - 1, -1, -1):
        tot += terms[k]
    assert (s.k1, s.k2, s.beta) == tuple(-tot[:3] / CF.mu) and s.storage == (-tot[3] / q["dt"], -tot[4] / q["dt"])
    assert s.mu == (CF.k1 * tot[0] + CF.k2 * tot[1] + CF.beta * tot[2]) / CF.mu ** 2 and s.mu != 0.0
    # ... and the restatement
    E, _ = A.point_matrix(o.CELL_QUAD, 1, 6, 5, 0, q["pts"])
    dJh = dJ.cpu().numpy()
    G = np.stack([np.concatenate([E.T @ dJh[k, :, 0], E.T @ dJh[k, :, 1]]) for k in range(N + 1)])
    sweep = A.adjoint_sweep(q["K"], q["M"], CF, q["storage"], q["theta"], q["dt"], q["masks"], list(traj.cpu().numpy()), G)
    ref = A.gradients(q["K"], q["M"], CF, q["storage"], q["dt"], q["masks"], G, sweep)
    et = float((np.abs(s.terms - sweep["terms"]) / sweep["sums"]).max())
    eq = float(np.abs(s.initial.vector() - ref["initial"]).max() / np.abs(ref["initial"]).max())
    bc = np.concatenate([f.vector() for f in s.bcs])
    eb = float(np.abs(bc - ref["bc"]).max() / np.abs(ref["bc"]).max())
    print(f"transient_sensitivities against the restatement on the recorded trajectory: terms {et:.2e}, initial {eq:.2e}, "
          f"boundary gradient {eb:.2e} (bar {LOOP_BAR:g})")
    assert et <= LOOP_BAR and eq <= LOOP_BAR and eb <= LOOP_BAR
    # point_sources is the transpose of Function.at
    u = fd.Function(q["V"], rng.standard_normal(n))
    c = rng.standard_normal(len(q["pts"]))
    b = fd.point_sources(q["V"], q["pts"], c)
    assert isinstance(b, np.ndarray) and abs(c @ u.at(q["pts"]) - b @ u.vector()) <= 1e-13 * (abs(c) @ (abs(E) @ abs(u.vector())))
    bd = fd.point_sources(q["V"], torch.from_numpy(q["pts"]).cuda(), torch.from_numpy(c).cuda())
    assert bd.is_cuda and np.array_equal(bd.cpu().numpy(), b)


def test_backward_through_the_transient_solve():
    import perphil_amd as pa
    from perphil_amd import transient

    q = _public_problem()
    W, N, n = q["W"], q["N"], q["n"]
    vals = (CF.k1, CF.k2, CF.beta, CF.mu) + q["storage"]
    k1, k2, beta, mu, S1 = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in vals[:5])
    S2 = torch.tensor(vals[5], dtype=torch.float64, device="cuda", requires_grad=True)
    init = torch.from_numpy(q["p0"]).cuda().requires_grad_()
    data = torch.from_numpy(np.random.default_rng(4).standard_normal((N + 1, len(q["pts"]), 2))).cuda()
    obs = transient.solve_dpp_transient_torch(W, k1, k2, beta, mu, S1, S2, q["bcs"], init, q["dt"], N, q["theta"], q["sp"],
                                              observe_at=q["pts"])
    assert obs.is_cuda and tuple(obs.shape) == (N + 1, len(q["pts"]), 2) and obs.requires_grad
    loss = 0.5 * torch.sum((obs - data) ** 2)
    # a forward solve with other parameters in between
    pa.solve_dpp_transient(W, pa.DPPParameters(k1=2.0, k2=0.5, beta=0.1, mu=1.0), q["bcs"], q["p0"], 0.1, 2, storage=(1.0, 1.0),
                           solver_parameters=q["sp"])
    loss.backward()
    # the explicit call on the same numbers
    ts = pa.solve_dpp_transient(W, q["params"], q["bcs"], init.detach(), q["dt"], N, storage=q["storage"], theta=q["theta"],
                                solver_parameters=q["sp"], on_device=True, record_trajectory=True)
    s = transient.transient_sensitivities(W, q["params"], q["bcs"], ts, dJ_dobs=(obs.detach() - data), observe_at=q["pts"],
                                          storage=q["storage"], theta=q["theta"], dt=q["dt"], solver_parameters=q["sp"])
    got = [t.grad for t in (k1, k2, beta, mu, S1, S2)]
    want = (s.k1, s.k2, s.beta, s.mu, s.storage[0], s.storage[1])
    print(f"autograd: {[float(t) for t in got]} / {want}")
    assert all(float(t) == v for t, v in zip(got, want))
    assert all(t.device == src.device for t, src in zip(got, (k1, k2, beta, mu, S1, S2))) and S2.grad.is_cuda
    assert init.grad.is_cuda and torch.equal(init.grad, s.initial.torch())
    # the final state as output
    pN = transient.solve_dpp_transient_torch(W, k1, k2, beta, mu, S1, S2, q["bcs"], q["p0"], q["dt"], N, q["theta"], q["sp"])
    assert pN.is_cuda and tuple(pN.shape) == (2 * n,) and torch.equal(pN.detach(), ts.trajectory[-1])


# ---- refusals through the C ABI -----------------------------------------------------------------------------------------------------
def test_adjoint_refusals_leave_the_context_usable(gpu_ctx_factory):
    kind, nx, ny = o.CELL_QUAD, 4, 4
    om = o.build_mesh(2, kind, nx, ny)
    n = om.num_nodes
    b = o.boundary_nodes(om)
    ctx = TG._shifted_context(gpu_ctx_factory, kind, nx, ny, 0, (b, b), (np.zeros(n), np.zeros(n)))
    cfg = TG._cfg(spar.CG_JACOBI_PARAMS)
    N = 2
    traj = np.random.default_rng(1).standard_normal((N + 1, 2 * n))
    G = np.ones((N + 1, 2 * n))
    with pytest.raises(ValueError, match="before pph_transient_begin"):
        ctx.transient_adjoint(cfg, traj, g=G)
    ctx.transient_begin(1.0, 0.5, 2.0, 1.0, (1.0, 2.0), 1.0, 0.1)
    terms, q0 = np.zeros((N, 5)), np.zeros(2 * n)
    done = C.c_int(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = _ffi.lib
    for fn in (lib.pph_transient_adjoint, lib.pph_transient_adjoint_device):
        for args in ((None, ptr(G), None, 0, None, 1e-12, N, ptr(terms), ptr(q0), None, None, C.byref(done)),
                     (ptr(traj), ptr(G), None, 0, None, 1e-12, N, None, ptr(q0), None, None, C.byref(done)),
                     (ptr(traj), ptr(G), None, 0, None, 1e-12, N, ptr(terms), None, None, None, C.byref(done))):
            assert fn(ctx._h, C.byref(cfg), *args) == _ffi.PPH_ERR_INVALID
            assert b"NULL buffer" in lib.pph_last_error(ctx._h)
        assert fn(ctx._h, C.byref(cfg), ptr(traj), None, None, 0, None, 1e-12, N, ptr(terms), ptr(q0), None, None,
                  C.byref(done)) == _ffi.PPH_ERR_INVALID
        assert b"neither g nor the observation form" in lib.pph_last_error(ctx._h)
        assert fn(ctx._h, C.byref(cfg), ptr(traj), ptr(G), None, 0, None, 1e-12, 0, ptr(terms), ptr(q0), None, None,
                  C.byref(done)) == _ffi.PPH_ERR_INVALID
        assert b"nsteps" in lib.pph_last_error(ctx._h)
    out5 = (C.c_double * 5)()
    assert lib.pph_transient_bilinear(ctx._h, None, ptr(q0), ptr(q0), 1.0, out5) == _ffi.PPH_ERR_INVALID
    nout = C.c_int64()
    assert lib.pph_eval_points_adjoint(ctx._h, None, 1, None, 1, 1e-12, ptr(q0), C.byref(nout)) == _ffi.PPH_ERR_INVALID
    assert lib.pph_eval_points_adjoint(ctx._h, ptr(q0), 1, ptr(q0), 1, 0.7, ptr(q0), C.byref(nout)) == _ffi.PPH_ERR_INVALID
    assert lib.pph_transient_steps_record_device(ctx._h, C.byref(cfg), ptr(q0), 1, 0.0, None, None, C.byref(done), None) == _ffi.PPH_ERR_INVALID
    assert lib.pph_transient_steps_record(ctx._h, C.byref(cfg), ptr(q0), 1, 0.0, None, None, C.byref(done), None) == _ffi.PPH_ERR_INVALID
    with pytest.raises(ValueError, match="neither g nor"):
        ctx.transient_adjoint(cfg, traj)
    ctx.assemble(1.0, 0.5, 2.0, 1.0)
    with pytest.raises(ValueError, match="assembled again"):
        ctx.transient_adjoint(cfg, traj, g=G)
    ctx.transient_begin(1.0, 0.5, 2.0, 1.0, (1.0, 2.0), 1.0, 0.1)
    ctx.set_dirichlet(1, b[:-1], np.zeros(len(b) - 1))
    with pytest.raises(ValueError, match="assembled again|Dirichlet sets changed"):
        ctx.transient_adjoint(cfg, traj, g=G)
    # ... and still works
    ctx.transient_begin(1.0, 0.5, 2.0, 1.0, (1.0, 2.0), 1.0, 0.1)
    terms, q0, wsum, infos, k = ctx.transient_adjoint(cfg, traj, g=G)
    assert k == N and all(i.converged for i in infos) and np.all(np.isfinite(terms)) and np.all(np.isfinite(q0))


def test_c_abi_refuses_slab_contexts():
    """Two ranks over gloo, each with its slab of a distributed mesh (world = 2): the entry points of the transient adjoint
    return PPH_ERR_INVALID with their message (tools/transient_adjoint_slab_check.py)."""
    import socket
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tools", "transient_adjoint_slab_check.py")]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0 and "world=2 transient adjoint refusals: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
