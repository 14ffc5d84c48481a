"""The restatement of the transient adjoint (tests/transient_adjoint_reference.py) against central differences of
``transient_reference.theta_steps``, the restated point evaluation against its transpose, and every refusal of the Python
surface - all without a GPU.

Finite differences: J = sum_s <C_s, p_s> with fixed random C_s (so G_s = C_s), relative step 1e-6, central.  Bar 1e-5 relative:
it is about the truncation and cancellation of the finite difference (about eps / step = 2e-10 relative to J, divided by the
relative size of the derivative), not about the recursion - the measured worst case over every case below is recorded in
tests/README_transient_adjoint.md.  Every test prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import dpp_oracle as o  # noqa: E402
import cmg_reference as CR  # noqa: E402
import transient_adjoint_reference as A  # noqa: E402
import transient_reference as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(o.CELL_QUAD, 5, 3, 0), (o.CELL_TRI, 4, 3, 0), (o.CELL_HEX, 3, 4, 2), (o.CELL_TET, 3, 2, 3)]
NAMES = ("quad", "tri", "hex", "tet")
FD_BAR = 1e-5
N_STEPS = 5


def _dim(kind):
    return 2 if kind in (o.CELL_QUAD, o.CELL_TRI) else 3


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{NAMES[c[0]]}{c[1]}x{c[2]}x{c[3]}")
def test_restatement_against_central_differences(case, theta):
    kind, nx, ny, nz = case
    om, K, M = T.scalar_matrices(_dim(kind), kind, nx, ny, nz)
    n = om.num_nodes
    nodes = CR.mixed_nodes(kind, nx, ny, nz)
    masks = T.masks_of(n, *nodes)
    con = np.concatenate(masks)
    rng = np.random.default_rng(31 + kind)
    g = (np.zeros(n), np.zeros(n))
    for f in (0, 1):
        g[f][nodes[f]] = rng.uniform(0.5, 1.5, len(nodes[f]))
    p0 = rng.standard_normal(2 * n)
    Cs = rng.standard_normal((N_STEPS + 1, 2 * n))
    base = dict(k1=1.3, k2=0.02, beta=3.0, mu=2.0, S1=0.3, S2=5.0)
    dt = 0.02

    def J(par, p_init=p0, data=g):
        cf = T.Coefs(par["k1"], par["k2"], par["beta"], par["mu"])
        states, _, _ = T.theta_steps(K, M, cf, (par["S1"], par["S2"]), theta, dt, masks, data, p_init, N_STEPS)
        return float(sum(Cs[s] @ states[s] for s in range(N_STEPS + 1)))

    cf = T.Coefs(base["k1"], base["k2"], base["beta"], base["mu"])
    states, _, _ = T.theta_steps(K, M, cf, (base["S1"], base["S2"]), theta, dt, masks, g, p0, N_STEPS)
    sweep = A.adjoint_sweep(K, M, cf, (base["S1"], base["S2"]), theta, dt, masks, states, Cs)
    grad = A.gradients(K, M, cf, (base["S1"], base["S2"]), dt, masks, Cs, sweep)
    assert np.all(grad["initial"][con] == 0.0) and all(np.all(w[con] == 0.0) for w in sweep["w"])
    assert np.all(grad["bc"][~con] == 0.0)
    h = 1e-6
    worst = 0.0
    for name in ("k1", "k2", "beta", "mu", "S1", "S2"):
        up, dn = dict(base), dict(base)
        up[name] *= 1 + h
        dn[name] *= 1 - h
        fd = (J(up) - J(dn)) / (2 * h * base[name])
        rel = abs(fd - grad[name]) / abs(grad[name])
        worst = max(worst, rel)
        print(f"{name}: adjoint {grad[name]:.9e}, central difference {fd:.9e}, relative {rel:.2e}")
    dp = np.where(con, 0.0, rng.standard_normal(2 * n))      # a free-dof direction of p_0
    fd = (J(base, p0 + h * dp) - J(base, p0 - h * dp)) / (2 * h)
    an = float(grad["initial"] @ dp)
    worst = max(worst, abs(fd - an) / abs(an))
    print(f"initial direction: adjoint {an:.9e}, central difference {fd:.9e}, relative {abs(fd - an) / abs(an):.2e}")
    dg = np.where(con, rng.uniform(-1.0, 1.0, 2 * n), 0.0)   # a direction of the boundary data
    gp = (g[0] + h * dg[:n], g[1] + h * dg[n:])
    gm = (g[0] - h * dg[:n], g[1] - h * dg[n:])
    fd = (J(base, p0, gp) - J(base, p0, gm)) / (2 * h)
    an = float(grad["bc"] @ dg)
    worst = max(worst, abs(fd - an) / abs(an))
    print(f"boundary direction: adjoint {an:.9e}, central difference {fd:.9e}, relative {abs(fd - an) / abs(an):.2e}")
    print(f"{NAMES[kind]} theta {theta}: worst relative discrepancy {worst:.2e} (bar {FD_BAR:g})")
    assert worst <= FD_BAR
    assert abs(grad["mu"]) > 0.0      # (mu sets the time scale: not the free zero of the steady case)


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{NAMES[c[0]]}{c[1]}x{c[2]}x{c[3]}")
def test_restated_evaluation_and_its_transpose(case, degree):
    """<c, E u> = <E^T c, u>, E against the restated evaluation of tests/point_eval_reference.py."""
    import point_eval_reference as P

    kind, nx, ny, nz = case
    rng = np.random.default_rng(3)
    pts = np.concatenate([P.random_points(kind, degree, 40), P.deliberate_points(kind, nx, ny, nz)[:40],
                          np.full((1, _dim(kind)), 1.5)])
    E, outside = A.point_matrix(kind, degree, nx, ny, nz, pts)
    nn = P.n_nodes(kind, degree, nx, ny, nz)
    u, c = rng.standard_normal(nn), rng.standard_normal(len(pts))
    ref = P.evaluate_fast(kind, degree, nx, ny, nz, u, pts, gradient=False)
    inside = ~outside
    assert outside[-1] and np.array_equal(outside, ref["outside"]) and E[outside].nnz == 0
    v = np.asarray(ref["v"][:, 0], dtype=np.float64)
    assert np.allclose((E @ u)[inside], v[inside], rtol=0, atol=1e-13 * abs(u).max())
    lhs, rhs = c[inside] @ (E @ u)[inside], (E.T @ c) @ u
    print(f"{NAMES[kind]} degree {degree}: <c, E u> - <E^T c, u> = {lhs - rhs:.2e}")
    assert abs(lhs - rhs) <= 1e-13 * (abs(c) @ (abs(E) @ abs(u)))
    assert np.allclose(np.asarray(E.sum(axis=1)).ravel()[inside], 1.0, atol=1e-14)      # partition of unity


def test_entry_points_are_declared_and_bound():
    from perphil_amd import _ffi

    header = open(os.path.join(ROOT, "include", "perphil_hip.h")).read()
    for name in ("pph_transient_bilinear", "pph_eval_points_adjoint", "pph_transient_steps_record", "pph_transient_adjoint"):
        for nm in (name, name + "_device"):
            assert nm in _ffi.EXPORTS and f"int {nm}(" in header and hasattr(_ffi.lib, nm)
    for name in ("transient_bilinear", "eval_points_adjoint", "transient_adjoint"):
        assert callable(getattr(_ffi.Context, name))


def test_refusals_come_before_any_context():
    from perphil_amd import DPPParameters, fd, transient
    from perphil_amd.partition import make_slab

    P = DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
    mesh = fd.UnitSquareMesh(3, 2, quadrilateral=True, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    n2 = W.dim()
    bcs = [fd.DirichletBC(W.sub(0), 1.0), fd.DirichletBC(W.sub(1), 0.0)]
    ilu = {"ksp_type": "gmres", "pc_type": "ilu", "ksp_rtol": 1e-12}
    p0 = np.zeros(n2)
    # recording and a steady-state stop; the byte budget (the message names the size)
    with pytest.raises(ValueError, match="steady_tol"):
        transient.solve_dpp_transient(W, P, bcs, p0, 0.1, 4, solver_parameters=ilu, steady_tol=1e-3, record_trajectory=True)
    with pytest.raises(ValueError, match=f"{5 * n2 * 8} bytes"):
        transient.solve_dpp_transient(W, P, bcs, p0, 0.1, 4, solver_parameters=ilu, record_trajectory=True,
                                      max_trajectory_bytes=5 * n2 * 8 - 1)
    N = 3
    sol = transient.TransientSolution(times=0.1 * np.arange(N + 1), solution=fd.Function(W), iterations=np.zeros(N, dtype=np.int64),
                                      rhs_norms=np.zeros(N), increment_norms=np.zeros(N), observations=None,
                                      trajectory=np.zeros((N + 1, n2)))
    assert sol.steps_done == N
    kw = dict(storage=(1.0, 2.0), theta=1.0, dt=0.1, solver_parameters=ilu)
    good, pts = np.zeros((N + 1, n2)), np.array([[0.5, 0.5], [0.25, 0.75]])
    with pytest.raises(ValueError, match="dJ_dp, dJ_dobs or both"):
        transient.transient_sensitivities(W, P, bcs, sol, **kw)
    for bad in (np.zeros((N, n2)), np.zeros((N + 1, n2 + 1)), np.zeros(n2)):
        with pytest.raises(ValueError, match="dJ_dp must have shape"):
            transient.transient_sensitivities(W, P, bcs, sol, dJ_dp=bad, **kw)
    for bad in (np.zeros((N + 1, 2)), np.zeros((N + 1, 3, 2)), np.zeros((N, 2, 2)), np.zeros((N + 1, 2, 1))):
        with pytest.raises(ValueError, match="dJ_dobs must have shape"):
            transient.transient_sensitivities(W, P, bcs, sol, dJ_dobs=bad, observe_at=pts, **kw)
    with pytest.raises(ValueError, match="observe_at"):
        transient.transient_sensitivities(W, P, bcs, sol, dJ_dobs=np.zeros((N + 1, 2, 2)), **kw)
    with pytest.raises(ValueError, match="observe_at must have shape"):
        transient.transient_sensitivities(W, P, bcs, sol, dJ_dobs=np.zeros((N + 1, 2, 2)), observe_at=np.zeros((2, 3)), **kw)
    with pytest.raises(fd.PointNotInDomainError):
        transient.transient_sensitivities(W, P, bcs, sol, dJ_dobs=np.zeros((N + 1, 2, 2)), observe_at=pts + 1.0, **kw)
    no_traj = transient.TransientSolution(times=sol.times, solution=sol.solution, iterations=sol.iterations, rhs_norms=sol.rhs_norms,
                                          increment_norms=sol.increment_norms, observations=None)
    assert no_traj.trajectory is None
    with pytest.raises(ValueError, match="record_trajectory=True"):
        transient.transient_sensitivities(W, P, bcs, no_traj, dJ_dp=good, **kw)
    for bad_kw, msg in ((dict(kw, storage=(0.0, 1.0)), "storage"), (dict(kw, theta=0.3), "theta"), (dict(kw, dt=0.0), "dt")):
        with pytest.raises(ValueError, match=msg):
            transient.transient_sensitivities(W, P, bcs, sol, dJ_dp=good, **bad_kw)
    with pytest.raises(NotImplementedError):
        transient.transient_sensitivities(W, P, bcs, sol, dJ_dp=good, **dict(kw, solver_parameters={"ksp_type": "bcgs"}))
    with pytest.raises(ValueError, match="2-field"):
        transient.transient_sensitivities(V, P, bcs, sol, dJ_dp=good, **kw)
    # point_sources: shapes, and a point outside
    with pytest.raises(ValueError, match="points must have shape"):
        fd.point_sources(V, np.zeros((2, 3)), np.zeros(2))
    with pytest.raises(ValueError, match="weights must have shape"):
        fd.point_sources(V, pts, np.zeros(3))
    with pytest.raises(fd.PointNotInDomainError):
        fd.point_sources(V, pts + 1.0, np.zeros(2))
    with pytest.raises(ValueError, match="W.sub"):
        fd.point_sources(W, pts, np.zeros(2))
    assert mesh._ctx is None and not mesh.__dict__.get("_ctx_deg")
    # a distributed mesh (the slab of rank 0 of 2, set by hand: no process group in this test)
    cube = fd.UnitCubeMesh(2, 2, 4, hexahedral=True, comm=fd.COMM_SELF)
    Vc = fd.FunctionSpace(cube, "CG", 1)
    Wc = Vc * Vc
    cube._slab = make_slab(2, 2, 4, 2, 0)
    assert cube.distributed
    bc_c = [fd.DirichletBC(Wc.sub(0), 1.0), fd.DirichletBC(Wc.sub(1), 0.0)]
    sol_c = transient.TransientSolution(times=sol.times, solution=fd.Function(Wc), iterations=sol.iterations, rhs_norms=sol.rhs_norms,
                                        increment_norms=sol.increment_norms, observations=None,
                                        trajectory=np.zeros((N + 1, Wc.local_dim())))
    with pytest.raises(NotImplementedError, match="comm=fd.COMM_SELF"):
        transient.transient_sensitivities(Wc, P, bc_c, sol_c, dJ_dp=np.zeros((N + 1, Wc.local_dim())), **kw)
    with pytest.raises(NotImplementedError, match="comm=fd.COMM_SELF"):
        transient.solve_dpp_transient(Wc, P, bc_c, np.zeros(Wc.local_dim()), 0.1, 2, solver_parameters=ilu, record_trajectory=True)
    with pytest.raises(NotImplementedError, match="COMM_SELF"):
        fd.point_sources(Vc, np.zeros((1, 3)), np.zeros(1))
    assert cube._ctx is None
    # the frozen result class
    s = transient.TransientSensitivities(k1=1.0, k2=2.0, beta=3.0, mu=0.5, storage=(1.0, 2.0), initial=fd.Function(W))
    assert s.bcs is None and s.info == {} and s.terms is None
    with pytest.raises(Exception):
        s.k1 = 2.0
