"""CPU checks behind the sources of the transient runs (perphil_amd/csrc/pph_sources.hip, perphil_amd/transient.py): the
restatement of tests/transient_sources_reference.py against its own closed form and against finite differences of itself,
the partition of unity of point loads, and every refusal of solve_dpp_transient(sources=...) that comes before a context
exists (no GPU here: a context would raise RuntimeError)."""
import numpy as np
import pytest

from oracle import dpp_oracle as o

import point_eval_reference as PE
import transient_adjoint_reference as A
import transient_reference as T
import transient_sources_reference as S

CF = T.Coefs(1.3, 0.02, 3.0, 2.0)
KINDS = [(o.CELL_QUAD, 5, 3, 0), (o.CELL_TRI, 4, 3, 0), (o.CELL_HEX, 3, 4, 2), (o.CELL_TET, 3, 2, 3)]


def _dim(kind):
    return 2 if kind in (o.CELL_QUAD, o.CELL_TRI) else 3


@pytest.mark.parametrize("network", [0, 1])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("kind,nx,ny,nz", [(o.CELL_QUAD, 4, 4, 0), (o.CELL_HEX, 3, 3, 3), (o.CELL_QUAD, 5, 3, 0)])
def test_direct_stepping_with_a_sine_source_follows_the_closed_form(kind, nx, ny, nz, theta, network):
    """(c1, c2) phi under direct stepping with the load M phi e_f and rates that change every step equals the 2 x 2 recursion to
    1e-14 of the largest amplitude (splu on fewer than 100 dofs; the homogeneous case of test_transient_host.py holds 2e-15)."""
    dim = _dim(kind)
    om, K, M = T.scalar_matrices(dim, kind, nx, ny, nz)
    n = om.num_nodes
    bnd = o.boundary_nodes(om)
    masks = T.masks_of(n, bnd, bnd)
    phi = T.sine_mode(om)
    phi[bnd] = 0.0
    storage, dt, N = (0.3, 5.0), 0.05, 7
    rates = np.array([0.0, 1.0, -2.0, 0.5, 0.5, 3.0, 0.0, 1.5])[:, None]
    coef = S.coefficients(rates, theta)
    states, _, _ = S.theta_steps(K, M, CF, storage, theta, dt, masks, (np.zeros(n), np.zeros(n)), np.concatenate([phi, -0.5 * phi]), N,
                                 [S.mass_load(M, phi, network)], coef)
    amp = S.closed_form_source_amplitudes(dim, nx, ny, nz, CF, storage, theta, dt, (1.0, -0.5), coef[:, 0], network)
    scale = max(np.abs(a).max() for a in amp) * np.abs(phi).max()
    for s in range(N + 1):
        assert np.abs(states[s] - np.concatenate([amp[s][0] * phi, amp[s][1] * phi])).max() <= 1e-14 * scale, s
    # the source matters: without it the amplitudes are other numbers by far more than the bar
    plain = T.closed_form_amplitudes(T.amplification(*T.mode_eigenvalues(dim, nx, ny, nz), CF, storage, theta, dt), (1.0, -0.5), N)
    assert np.abs(plain[-1] - amp[-1]).max() > 1e-3


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("case", KINDS)
def test_point_loads_are_a_partition_of_unity(case, degree):
    """The entries of a point load sum to 1 (interior, face, edge, vertex, boundary and corner points), an outside point has an
    empty row, and at degree 1 the oracle's shape functions and the restated point evaluation give the same load."""
    kind, nx, ny, nz = case
    dim = _dim(kind)
    pts = np.concatenate([PE.random_points(kind, degree, 40), PE.deliberate_points(kind, nx, ny, nz), np.zeros((1, dim)), np.ones((1, dim)),
                          np.array([[1.5] + [0.5] * (dim - 1)])])
    fields = np.arange(len(pts)) % 2
    L, outside = S.point_loads(kind, degree, nx, ny, nz, pts, fields)
    n = L.shape[1] // 2
    assert outside[-1] and not outside[:-1].any() and not L[-1].any()
    for p in range(len(pts) - 1):
        mine, other = L[p, fields[p] * n:(fields[p] + 1) * n], L[p, (1 - fields[p]) * n:(2 - fields[p]) * n]
        assert abs(mine.sum() - 1.0) <= 64 * T.EPS and not other.any()      # (at most 27 basis values of magnitude <= 1)
    if degree == 1:
        E, out2 = A.point_matrix(kind, 1, nx, ny, nz, pts)
        rows = np.stack([L[p, fields[p] * n:(fields[p] + 1) * n] for p in range(len(pts))])
        assert np.array_equal(out2, outside) and np.abs(rows - E.toarray()).max() <= 8 * T.EPS


def test_rate_gradients_of_the_restatement_match_finite_differences():
    """G[s][k] = w_s^T F L_k and dJ/dr_k(t_j) = theta G[j-1][k] + (1 - theta) G[j][k] against central differences of the
    restatement's own J = sum_s <g_s, p_s>, which is linear in the rates: the difference quotient has no truncation error."""
    kind, nx, ny, nz = o.CELL_QUAD, 5, 3, 0
    om, K, M = T.scalar_matrices(2, kind, nx, ny, nz)
    n = om.num_nodes
    bnd = o.boundary_nodes(om)
    masks = T.masks_of(n, bnd[::2], bnd)
    g = (np.zeros(n), np.zeros(n))
    rng = np.random.default_rng(3)
    storage, theta, dt, N = (0.3, 5.0), 0.5, 0.02, 4
    pts = np.array([[0.31, 0.62], [0.8, 0.2], [0.4, 1.0 / 3.0]])
    loads = np.concatenate([S.point_loads(kind, 1, nx, ny, nz, pts, [0, 1, 1], om)[0], S.mass_load(M, rng.standard_normal(n), 0)[None]])
    rates = rng.standard_normal((N + 1, 4))
    gs = rng.standard_normal((N + 1, 2 * n))
    p0 = rng.standard_normal(2 * n)

    def J(r):
        st, _, _ = S.theta_steps(K, M, CF, storage, theta, dt, masks, g, p0, N, loads, S.coefficients(r, theta))
        return float(sum(gs[s] @ st[s] for s in range(N + 1)))

    states, _, _ = S.theta_steps(K, M, CF, storage, theta, dt, masks, g, p0, N, loads, S.coefficients(rates, theta))
    sweep = A.adjoint_sweep(K, M, CF, storage, theta, dt, masks, states, gs)
    G, _ = S.source_gradients(sweep, loads, masks)
    dr = S.rate_gradients(G, theta)
    for j, k in ((0, 0), (2, 1), (N, 3), (1, 2)):
        e = np.zeros_like(rates)
        e[j, k] = 1.0
        fd = (J(rates + e) - J(rates - e)) / 2.0
        assert abs(fd - dr[j, k]) <= 1e-10 * max(abs(fd), np.abs(dr).max()), (j, k, fd, dr[j, k])


# -- solve_dpp_transient(sources=...): everything that is refused before a context exists -----------------------------------
def _space(dim=2):
    from perphil_amd import fd

    mesh = fd.Mesh(2, fd.CELL_QUAD, 4, 4, 0, comm=fd.COMM_SELF) if dim == 2 else fd.Mesh(3, fd.CELL_HEX, 2, 2, 2, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(mesh, "CG", 1)
    return mesh, V, V * V


def _call(W, **kw):
    import perphil_amd as pa
    from perphil_amd import solver_parameters as spar

    n = W.sub(0).local_dim()
    args = dict(initial=np.zeros(2 * n), dt=0.1, num_steps=3, storage=(1.0, 2.0), theta=1.0, solver_parameters=spar.CG_JACOBI_PARAMS)
    args.update(kw)
    return pa.solve_dpp_transient(W, pa.DPPParameters(), [], **args)


def _refusals():
    from perphil_amd import fd
    from perphil_amd.transient import DistributedSource as D, Well as Wl

    ok = [0.5, 0.5]
    return [
        ("rate too short", dict(sources=[Wl(ok, np.ones(3))]), ValueError),
        ("rate too long", dict(sources=[Wl(ok, np.ones(5))]), ValueError),
        ("rate of two axes", dict(sources=[Wl(ok, np.ones((4, 1)))]), ValueError),
        ("rate no number", dict(sources=[Wl(ok, "fast")]), ValueError),
        ("nan rate", dict(sources=[Wl(ok, float("nan"))]), ValueError),
        ("inf in a schedule", dict(sources=[Wl(ok, np.array([0.0, 1.0, np.inf, 0.0]))]), ValueError),
        ("callable gives inf", dict(sources=[D(np.ones(25), lambda t: float("inf") if t > 0.15 else 1.0)]), ValueError),
        ("network 2", dict(sources=[Wl(ok, 1.0, network=2)]), ValueError),
        ("network -1", dict(sources=[D(np.ones(25), 1.0, network=-1)]), ValueError),
        ("point outside", dict(sources=[Wl([0.5, 1.5], 1.0)]), fd.PointNotInDomainError),
        ("point just outside", dict(sources=[Wl([-1e-6, 0.5], 1.0)]), fd.PointNotInDomainError),
        ("nan point", dict(sources=[Wl([float("nan"), 0.5], 1.0)]), fd.PointNotInDomainError),
        ("point of three coordinates", dict(sources=[Wl([0.5, 0.5, 0.5], 1.0)]), ValueError),
        ("steady_tol with a schedule", dict(sources=[Wl(ok, np.array([0.0, 1.0, 1.0, 1.0]))], steady_tol=1e-3), ValueError),
        ("steady_tol with a callable", dict(sources=[Wl(ok, 2.0), D(np.ones(25), lambda t: t)], steady_tol=1e-3), ValueError),
        ("f of a wrong length", dict(sources=[D(np.ones(24))]), ValueError),
        ("callable f of a wrong shape", dict(sources=[D(lambda X: X)]), ValueError),
        ("no source object", dict(sources=[(ok, 1.0)]), ValueError),
    ]


@pytest.mark.parametrize("index", range(18))
def test_solve_dpp_transient_refuses_sources_before_a_context(index):
    """Without the feature every one of these ends in a TypeError (no ``sources`` argument, no ``Well``)."""
    name, kw, exc = _refusals()[index]
    mesh, V, W = _space()
    with pytest.raises(exc) as e:
        _call(W, **kw)
    assert not isinstance(e.value, (RuntimeError, TypeError)), name


def test_refusal_list_is_complete():
    assert len(_refusals()) == 18


def test_sources_refusals_on_a_mixed_function_and_in_the_sensitivities():
    from perphil_amd import fd, transient

    mesh, V, W = _space()
    with pytest.raises(ValueError, match="scalar Function"):
        _call(W, sources=[transient.DistributedSource(fd.Function(W))])
    mesh3, V3, W3 = _space(3)
    with pytest.raises(ValueError, match="scalar Function"):
        _call(W, sources=[transient.DistributedSource(fd.Function(V3))])
    with pytest.raises(fd.PointNotInDomainError):
        _call(W3, initial=np.zeros(2 * 27), sources=[transient.Well([0.5, 0.5, 1.0 + 1e-9], 1.0)])
    # the plan: the caller's order against the library's (dense loads first), and the coefficient table
    plan = transient._plan_sources(W, 1, [transient.Well([0.5, 0.5], [0.0, 1.0, 2.0, 4.0], 1), transient.DistributedSource(np.ones(25), 3.0),
                                          transient.Well([0.0, 1.0], lambda t: 10.0 * t)], 3, 0.1, 0.5)
    assert plan.rates.shape == (4, 3) and plan.perm.tolist() == [1, 0, 2] and plan.fields.tolist() == [1, 0]
    assert np.allclose(plan.rates[:, 2], [0.0, 1.0, 2.0, 3.0]) and np.array_equal(plan.coef[:, 0], [3.0, 3.0, 3.0])
    assert np.array_equal(plan.coef[:, 1], [0.5, 1.5, 3.0]) and np.allclose(plan.coef[:, 2], [0.5, 1.5, 2.5])
    assert transient._plan_sources(W, 1, [], 3, 0.1, 1.0) is None and transient._plan_sources(W, 1, None, 3, 0.1, 1.0) is None
