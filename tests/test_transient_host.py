"""CPU checks behind the transient DPP path (perphil_amd/csrc/pph_transient.hip): the NumPy restatement of
tests/transient_reference.py against the closed form of the sine mode, the restated box matrices of the matrix-free step
kernel against the oracle's assembled K and M, and the binding of the new entry points."""
import numpy as np
import pytest

from oracle import dpp_oracle as o

import transient_reference as T

CF = T.Coefs(1.0, 0.01, 1.0, 1.0)


@pytest.mark.parametrize("kind,nx,ny,nz", [(o.CELL_QUAD, 4, 4, 0), (o.CELL_QUAD, 8, 8, 0), (o.CELL_HEX, 3, 3, 3), (o.CELL_HEX, 4, 4, 4),
                                           (o.CELL_QUAD, 5, 3, 0), (o.CELL_HEX, 3, 4, 2)])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("storage", [(1.0, 20.0), (0.3, 5.0)])
def test_direct_stepping_follows_the_closed_form(kind, nx, ny, nz, theta, storage):
    """(1, -0.5) phi under direct theta stepping equals G^n (1, -0.5) phi to 2e-15 relative, 9 steps."""
    dim = 2 if kind == o.CELL_QUAD else 3
    om, K, M = T.scalar_matrices(dim, kind, nx, ny, nz)
    n = om.num_nodes
    b = o.boundary_nodes(om)
    masks = T.masks_of(n, b, b)
    phi = T.sine_mode(om)
    phi[b] = 0.0   # (sin(pi) is 1.2e-16, not 0)
    lam_k, lam_m = T.mode_eigenvalues(dim, nx, ny, nz)
    f = ~masks[0]
    assert abs((K @ phi - lam_k * phi)[f]).max() <= 1e-14 * abs(lam_k * phi).max()
    assert abs((M @ phi - lam_m * phi)[f]).max() <= 1e-14 * abs(lam_m * phi).max()
    dt, nsteps = 0.05, 9
    G = T.amplification(lam_k, lam_m, CF, storage, theta, dt)
    amps = T.closed_form_amplitudes(G, (1.0, -0.5), nsteps)
    zeros = (np.zeros(n), np.zeros(n))
    states, bn, dn = T.theta_steps(K, M, CF, storage, theta, dt, masks, zeros, np.concatenate([phi, -0.5 * phi]), nsteps)
    assert len(states) == nsteps + 1 and bn.shape == dn.shape == (nsteps,)
    for s, c in zip(states, amps):
        ref = np.concatenate([c[0] * phi, c[1] * phi])
        err = abs(s - ref).max() / abs(np.concatenate([phi, -0.5 * phi])).max()
        print(f"kind {kind} {nx}x{ny}x{nz} theta {theta} S {storage}: {err:.2e}")
        assert err <= 2e-15


@pytest.mark.parametrize("kind,nx,ny,nz,least", [(o.CELL_TRI, 4, 4, 0, 0.01), (o.CELL_TET, 3, 3, 3, 0.01)])
def test_sine_mode_is_no_mass_eigenvector_on_simplices(kind, nx, ny, nz, least):
    """Why simplices are pinned by the restatement alone."""
    dim = 2 if kind == o.CELL_TRI else 3
    om, K, M = T.scalar_matrices(dim, kind, nx, ny, nz)
    phi = T.sine_mode(om)
    f = np.ones(om.num_nodes, dtype=bool)
    f[o.boundary_nodes(om)] = False
    phi[~f] = 0.0
    y = (M @ phi)[f]
    lam = (y @ phi[f]) / (phi[f] @ phi[f])
    assert abs(y - lam * phi[f]).max() / abs(y).max() >= least


CASES = [(o.CELL_QUAD, 5, 3, 0), (o.CELL_TRI, 4, 3, 0), (o.CELL_HEX, 5, 3, 4), (o.CELL_TET, 3, 4, 2), (o.CELL_QUAD, 1, 1, 0),
         (o.CELL_TET, 1, 2, 1)]


@pytest.mark.parametrize("kind,nx,ny,nz", CASES)
def test_box_matrices_assemble_the_oracles_K_and_M(kind, nx, ny, nz):
    """The closed-form box matrices the step kernel gathers from, summed over the existing boxes of every node, are the
    oracle's quadrature-assembled K and M (exact rules on these cells) to rounding; same pattern."""
    dim = 2 if kind in (o.CELL_QUAD, o.CELL_TRI) else 3
    om, K, M = T.scalar_matrices(dim, kind, nx, ny, nz)
    Kf, Mf = T.matfree_scalar_matrices(kind, nx, ny, nz)
    assert abs(Kf - K).max() <= 1e-13 * abs(K).max()
    assert abs(Mf - M).max() <= 1e-13 * abs(M).max()


def test_step_rhs_restatement_masks_and_bound():
    om, K, M = T.scalar_matrices(2, o.CELL_QUAD, 5, 3)
    n = om.num_nodes
    b = o.boundary_nodes(om)
    masks = T.masks_of(n, b, b[::2])
    p = np.random.default_rng(3).standard_normal(2 * n)
    r = T.step_rhs(K, M, CF, masks, p)
    assert np.all(r[np.concatenate(masks)] == 0.0)
    free = ~np.concatenate(masks)
    full = -(T.unel_operator(K, M, CF) @ p)
    assert np.array_equal(r[free], full[free])
    assert np.all(abs(full) <= T.abs_bound(K, M, CF, p) * (1 + 1e-14))


def test_launch_rule_of_the_step_kernel():
    assert not T.step_kernel_loops(2048 * 256) and T.step_kernel_loops(2048 * 256 + 1)
    assert T.step_kernel_loops(1025 * 513)


def test_binding_exposes_the_step_right_hand_side():
    from perphil_amd import _ffi

    for name in ("pph_dpp_step_rhs", "pph_dpp_step_rhs_device"):
        assert name in _ffi.EXPORTS and hasattr(_ffi.lib, name)
    assert callable(_ffi.Context.step_rhs)


# -- solve_dpp_transient: everything that is refused before a context exists (no GPU here: a context would raise RuntimeError) ----
def _space(degree=1):
    from perphil_amd import fd

    mesh = fd.Mesh(2, fd.CELL_QUAD, 4, 4, 0, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(mesh, "CG", degree)
    return mesh, V, V * V


def _call(W, **kw):
    import perphil_amd as pa
    from perphil_amd import solver_parameters as spar

    n = W.sub(0).local_dim()
    args = dict(initial=np.zeros(2 * n), dt=0.1, num_steps=2, storage=(1.0, 2.0), theta=1.0, solver_parameters=spar.CG_JACOBI_PARAMS)
    args.update(kw)
    return pa.solve_dpp_transient(W, pa.DPPParameters(), [], **args)


@pytest.mark.parametrize("kw,exc", [
    (dict(storage=(0.0, 1.0)), ValueError), (dict(storage=(1.0, float("inf"))), ValueError), (dict(storage=1.0), ValueError),
    (dict(dt=0.0), ValueError), (dict(dt=float("nan")), ValueError), (dict(theta=0.49), ValueError), (dict(theta=1.01), ValueError),
    (dict(num_steps=0), ValueError), (dict(record_every=-1), ValueError), (dict(initial=np.zeros(3)), ValueError),
    (dict(initial=(np.zeros(25), np.zeros(24))), ValueError), (dict(initial=(np.zeros(25),)), ValueError),
    (dict(observe_at=np.zeros((3, 3))), ValueError), (dict(solver_parameters={"ksp_type": "bcgs"}), NotImplementedError),
])
def test_solve_dpp_transient_refuses_before_a_context(kw, exc):
    mesh, V, W = _space()
    with pytest.raises(exc) as e:
        _call(W, **kw)
    assert not isinstance(e.value, RuntimeError) or "pph_ctx_create" not in str(e.value)


def test_solve_dpp_transient_keeps_the_degree_two_refusals():
    from perphil_amd import solver_parameters as spar

    mesh, V, W = _space(degree=2)
    n = W.sub(0).local_dim()
    for params in (spar.CG_CMG_PARAMS, spar.FIELDSPLIT_MG_PARAMS):
        with pytest.raises(NotImplementedError):
            _call(W, initial=np.zeros(2 * n), solver_parameters=params)
    import perphil_amd as pa

    with pytest.raises(ValueError):
        pa.solve_dpp_transient(V, pa.DPPParameters(), [], np.zeros(n), 0.1, 1)


def test_solve_dpp_transient_refuses_a_distributed_mesh():
    """The slab of rank 0 of 2, set by hand (no process group in this test), as tests/test_adjoint_host.py does."""
    import perphil_amd as pa
    from perphil_amd import fd, solver_parameters as spar
    from perphil_amd.partition import make_slab

    cube = fd.UnitCubeMesh(2, 2, 4, hexahedral=True, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(cube, "CG", 1)
    W = V * V
    cube._slab = make_slab(2, 2, 4, 2, 0)
    assert cube.distributed
    bcs = [fd.DirichletBC(W.sub(0), 1.0), fd.DirichletBC(W.sub(1), 0.0)]
    with pytest.raises(NotImplementedError, match="comm=fd.COMM_SELF"):
        pa.solve_dpp_transient(W, pa.DPPParameters(), bcs, np.zeros(W.local_dim()), 0.1, 2, solver_parameters=spar.CG_JACOBI_PARAMS)
    assert cube._ctx is None


def test_transient_solution_shapes():
    from perphil_amd import fd
    from perphil_amd.transient import TransientSolution

    mesh, V, W = _space()
    n = W.sub(0).local_dim()
    f = fd.Function(W, np.zeros(2 * n))
    t = TransientSolution(times=0.1 * np.arange(4), solution=f, iterations=np.array([3, 2, 2]), rhs_norms=np.ones(3),
                          increment_norms=np.ones(3), observations=np.zeros((4, 5, 2)), snapshots={0: f, 3: f})
    assert t.steps_done == 3 and t.times.shape == (4,) and t.iterations.shape == t.rhs_norms.shape == t.increment_norms.shape == (3,)
    assert t.observations.shape == (4, 5, 2) and sorted(t.snapshots) == [0, 3]
