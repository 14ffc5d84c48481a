"""Coupled multigrid (pc_type pph_cmg, perphil_amd/csrc/pph_cmg.hip) on the device.

1. the cycle itself: pph_pc_apply_coupled against the fp64 restatement (tests/cmg_reference.py) on a random vector and on
   vectors on which one level dominates, max |z - ref| <= CYCLE_BOUND max |ref|; at beta = 1e4 the bound is 100 x the drift
   between the restatement in float64 and in longdouble, at least CYCLE_BOUND;
2. different Dirichlet sets per field, then other sets and other coefficients on the same context;
3. operator formats: op_format, asm_store_values, mg_fused;
4. the grid-stride paths of the row-walk and node kernels, the second trip of the one-workgroup coarsest solve's loops, the
   host-driven coarsest solve, and coarsest solves that stop short on either path (inner_failed);
5. solves through solve_dpp against the oracle's direct solve and the restatement's CG counts;
6. condition numbers against the dense eig(B A) of the restatement;
7. refusals at the C level.
tests/test_cmg_host.py shows that comparison 1 rejects cycles that are wrong by a little."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cmg_reference as C  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

import perphil_amd as pa  # noqa: E402
from perphil_amd import _ffi, conditioning, convergence_2d as c2, fd, solver_parameters as spar  # noqa: E402
from perphil_amd.solver import translate_options  # noqa: E402

pytestmark = pytest.mark.gpu

R = C.R
K1, K2, MU = C.K1, C.K2, C.MU
_cache = {}


def _nodes(kind, nx, ny, nz, sets):
    if sets == "boundary":
        b = R.dirichlet_nodes(kind, nx, ny, nz, 1)
        return b, b
    return C.mixed_nodes(kind, nx, ny, nz, second=(sets == "mixed2"))


def _levels(kind, nx, ny, nz, beta, sets="boundary", k1=K1, k2=K2):
    key = (kind, nx, ny, nz, beta, sets, k1, k2)
    if key not in _cache:
        n = R.level_nodes(kind, nx, ny, nz)[0]
        _cache[key] = C.coupled_hierarchy(kind, nx, ny, nz, C.masks_from_nodes(n, _nodes(kind, nx, ny, nz, sets)), k1=k1, k2=k2, beta=beta)
    return _cache[key]


def _assemble(ctx, kind, nx, ny, nz, beta, sets="boundary", k1=K1, k2=K2):
    nodes = _nodes(kind, nx, ny, nz, sets)
    for f in (0, 1):
        ctx.set_dirichlet(f, nodes[f], R.dirichlet_values(kind, nx, ny, nz, nodes[f], f))
    ctx.assemble(k1, k2, beta, MU, monolithic=True)


def _open(kind, nx, ny, nz, options=()):
    ctx = _ffi.Context(0)
    for name, value in options:
        ctx.set_option(name, value)
    ctx.mesh_build(R.dim_of(kind), kind, nx, ny, nz)
    return ctx


def _check_cycle(ctx, lv, label, smooths=(1, 2, 3), bound=C.CYCLE_BOUND, seed=11, vectors=None):
    mask = np.concatenate(lv[0].mask)
    vectors = vectors if vectors is not None else C.probe_vectors(lv, seed)
    out = {}
    for ns in smooths:
        worst = (0.0, "")
        for name, r in vectors:
            ref = C.apply_reference(lv, r, ns)
            rd = r.copy()
            rd[mask] = 7.0                                     # the entry point clears constrained entries itself
            z = ctx.pc_apply_coupled(_ffi.PC_CMG, rd, mg_smooth=ns)
            err = C.rel_err(z, ref)
            worst = max(worst, (err, name))
            print(f"{label}: levels {[L.n for L in lv]} mg_smooth {ns} {name}: |z - ref| / |ref| = {err:.2e}, bound {bound:.1e}")
            assert err <= bound, (label, ns, name, err)
            assert not z[mask].any()
            if name.startswith("random"):
                assert np.array_equal(z, ctx.pc_apply_coupled(_ffi.PC_CMG, rd, mg_smooth=ns))
        out[ns] = worst[0]
    return out


MESHES = {"quad16x12": (C.QUAD, 16, 12, 0), "tri12": (C.TRI, 12, 12, 0), "hex8": (C.HEX, 8, 8, 8), "tet4": (C.TET, 4, 4, 4),
          "quad5": (C.QUAD, 5, 5, 0)}
NLEV = {"quad16x12": 3, "tri12": 3, "hex8": 3, "tet4": 2, "quad5": 1}


# ---- 1. the cycle itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [C.BETA, 1e2])
@pytest.mark.parametrize("name", list(MESHES))
def test_cycle_against_the_restatement(name, beta):
    kind, nx, ny, nz = MESHES[name]
    lv = _levels(kind, nx, ny, nz, beta)
    assert len(lv) == NLEV[name]          # (quad 16 x 12: three levels, 4 x 3 stops; quad 5 x 5: the Chebyshev-only rule)
    with _open(kind, nx, ny, nz) as ctx:
        _assemble(ctx, kind, nx, ny, nz, beta)
        A = ctx.csr(_ffi.MAT_MONO)
        assert abs(A - lv[0].A).max() <= 1e-12 * abs(lv[0].A).max()
        _check_cycle(ctx, lv, f"{name} beta {beta:g}")


@pytest.mark.parametrize("name", list(MESHES))
def test_cycle_at_large_exchange(name):
    """beta = 1e4: bound = 100 x the drift between the restatement in float64 and in longdouble, at least CYCLE_BOUND."""
    kind, nx, ny, nz = MESHES[name]
    lv = _levels(kind, nx, ny, nz, 1e4)
    vectors = C.probe_vectors(lv, 13)
    lq = C.levels_as(lv, np.longdouble)
    with _open(kind, nx, ny, nz) as ctx:
        _assemble(ctx, kind, nx, ny, nz, 1e4)
        for ns in (1, 2, 3):
            drift = max(C.rel_err(C.apply_reference(lv, r, ns), C.apply_reference(lq, r, ns).astype(np.float64)) for _n, r in vectors)
            bound = max(100 * drift, C.CYCLE_BOUND)
            print(f"{name} beta 1e4 mg_smooth {ns}: drift float64 / longdouble {drift:.2e}, bound {bound:.2e}")
            _check_cycle(ctx, lv, f"{name} beta 1e4", smooths=(ns,), bound=bound, vectors=vectors)


# ---- 2. different Dirichlet sets per field, and a context that is assembled again ----------------------------------------
@pytest.mark.parametrize("name", ["quad16x12", "hex8"])
def test_different_dirichlet_sets_and_reassembly(name):
    kind, nx, ny, nz = MESHES[name]
    with _open(kind, nx, ny, nz) as ctx:
        lv = _levels(kind, nx, ny, nz, 1e2, "mixed")
        m0, m1 = lv[0].mask
        assert (m0 != m1).any() and any((L.mask[0] != L.mask[1]).any() for L in lv[1:])   # degenerate blocks on coarse levels too
        _assemble(ctx, kind, nx, ny, nz, 1e2, "mixed")
        _check_cycle(ctx, lv, f"{name} mixed sets", smooths=(1, 2))
        # other coefficients, same sets: the coupled set-up follows the assembly
        lv = _levels(kind, nx, ny, nz, 30.0, "mixed", k1=0.3, k2=2.0)
        _assemble(ctx, kind, nx, ny, nz, 30.0, "mixed", k1=0.3, k2=2.0)
        _check_cycle(ctx, lv, f"{name} mixed sets, k1 0.3 k2 2 beta 30", smooths=(2,), seed=12)
        # other sets and other coefficients
        lv = _levels(kind, nx, ny, nz, 5.0, "mixed2", k1=2.0, k2=0.05)
        _assemble(ctx, kind, nx, ny, nz, 5.0, "mixed2", k1=2.0, k2=0.05)
        _check_cycle(ctx, lv, f"{name} second sets, k1 2 k2 0.05 beta 5", smooths=(1, 2), seed=13)


def test_a_cycle_leaves_the_assembly_path_alone():
    """The cycle integrates K and M of every level for itself: the context's own assembly - fused, nothing kept - and what is
    solved from it keep their bits after a coupled cycle has run on the context."""
    kind, nx, ny, nz = MESHES["hex8"]
    cfg, _ = translate_options(spar.FIELDSPLIT_MG_PARAMS)
    with _open(kind, nx, ny, nz) as ctx:
        def state():
            _assemble(ctx, kind, nx, ny, nz, 1e2)
            t = ctx.timers()
            x, info, _ = ctx.solve(cfg)
            assert info.converged
            return (t["asm_rows"], t["asm_rows_straight"], t["asm_rows_general"]), [ctx.csr(m).data.copy() for m in (_ffi.MAT_A11, _ffi.MAT_A22, _ffi.MAT_A12)], x.copy()
        rows0, mats0, x0 = state()
        _assemble(ctx, kind, nx, ny, nz, 1e2)
        ctx.pc_apply_coupled(_ffi.PC_CMG, np.ones(2 * ctx.n))
        rows1, mats1, x1 = state()
        assert rows0 == rows1
        assert all(np.array_equal(a, b) for a, b in zip(mats0, mats1)) and np.array_equal(x0, x1)


# ---- 3. operator formats ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quad16x12", "hex8"])
def test_operator_formats(name):
    kind, nx, ny, nz = MESHES[name]
    lv = _levels(kind, nx, ny, nz, 1e2, "mixed")
    vectors = C.probe_vectors(lv, 17)
    res = {}
    for op_format in (0, 1):
        for store in (0, 1):
            for fused in (0, 1):
                opts = (("op_format", op_format), ("asm_store_values", store), ("mg_fused", fused), ("sell_dict_min_rows", 1))
                with _open(kind, nx, ny, nz, opts) as ctx:
                    _assemble(ctx, kind, nx, ny, nz, 1e2, "mixed")
                    _check_cycle(ctx, lv, f"{name} op_format {op_format} store {store} fused {fused}", smooths=(2,), vectors=vectors)
                    res[(op_format, store, fused)] = [ctx.pc_apply_coupled(_ffi.PC_CMG, r, mg_smooth=2) for _n, r in vectors]
    for op_format in (0, 1):
        base = res[(op_format, 0, 0)]
        for store in (0, 1):
            for fused in (0, 1):
                assert all(np.array_equal(a, b) for a, b in zip(base, res[(op_format, store, fused)])), (op_format, store, fused)
    for a, b in zip(res[(0, 0, 0)], res[(1, 0, 0)]):
        assert C.rel_err(a, b) <= C.FUSED_BOUND


# ---- 4. grid-stride paths and the host-driven coarsest solve -----------------------------------------------------------------
@pytest.mark.parametrize("name,kind,nx,ny,nz,what", [
    ("hex40", C.HEX, 40, 40, 40, "rows"),          # 41^3 = 68 921 rows > 65 536: k_cmg_row<8> and k_cmg_setup<8> loop
    ("quad368", C.QUAD, 368, 368, 0, "rows"),      # 369^2 = 136 161 rows > 131 072: the 4-lane kernels loop (363^2 would do, but
                                                   # 368 = 16 x 23 coarsens to a level the one-workgroup CG takes)
    ("quad512", C.QUAD, 512, 512, 0, "nodes"),     # 513^2 = 263 169 nodes > 262 144: k_cmg_init and k_cmg_mask_copy loop
    ("quad130", C.QUAD, 130, 130, 0, "coarse"),    # 130 -> 65 stops: a coarsest level of 66^2 = 4 356 nodes > 4 096
    ("quad126", C.QUAD, 126, 126, 0, "onchip"),    # 126 -> 63 stops: 64^2 = 4 096 nodes, the largest k_cmg_coarse_cg takes: four
                                                   # trips of its 1 024 threads through every loop
    ("hex30", C.HEX, 30, 30, 30, "onchip"),        # 30 -> 15 stops: 16^3 = 4 096 nodes, 27-entry rows
])
def test_launch_branches(name, kind, nx, ny, nz, what):
    ns = R.level_nodes(kind, nx, ny, nz)
    if what == "rows":
        assert C.row_kernel_loops(kind, ns[0]) and not C.node_kernel_loops(ns[0]) and ns[-1] <= C.CMG_COARSE_ONCHIP
        smaller = (38, 38, 38) if kind == C.HEX else (360, 360, 0)     # the next mesh down with such a hierarchy does not loop
        assert not C.row_kernel_loops(kind, R.level_nodes(kind, *smaller)[0])
    elif what == "nodes":
        assert C.node_kernel_loops(ns[0]) and not C.node_kernel_loops(R.level_nodes(kind, nx - 1, ny - 1, 0)[0])
    elif what == "onchip":
        assert len(ns) == 2 and C.COARSE_THREADS < ns[-1] <= C.CMG_COARSE_ONCHIP
    else:
        assert len(ns) == 2 and ns[-1] > C.CMG_COARSE_ONCHIP and R.level_nodes(kind, 126, 126, 0)[-1] <= C.CMG_COARSE_ONCHIP
    t0 = time.time()
    lv = _levels(kind, nx, ny, nz, 1e2, "mixed")
    t1 = time.time()
    with _open(kind, nx, ny, nz) as ctx:
        _assemble(ctx, kind, nx, ny, nz, 1e2, "mixed")
        _check_cycle(ctx, lv, f"{name} ({what} branch)", smooths=(2,), vectors=C.probe_vectors(lv, 19)[:2])
    _cache.clear()
    print(f"{name}: restatement {t1 - t0:.1f} s, device + comparison {time.time() - t1:.1f} s")


@pytest.mark.parametrize("on_device", [1, 0])
def test_a_coarsest_solve_that_stops_short_is_reported(on_device):
    """coarse_max_it 2 on a coarsest level of 20 nodes: the one-workgroup CG (its record on the device) and the host-driven
    CG (option coarse_on_device 0) both stop short and the solve says inner_failed; an application outside a solve leaves
    nothing behind for the next solve, and a solve with the default limit is clean again."""
    kind, nx, ny, nz = MESHES["quad16x12"]
    lv = _levels(kind, nx, ny, nz, 1e2)
    assert lv[-1].n == 20
    cfg, _ = translate_options(spar.CG_CMG_PARAMS)
    with _open(kind, nx, ny, nz, (("coarse_on_device", on_device),)) as ctx:
        _assemble(ctx, kind, nx, ny, nz, 1e2)
        _x, info, _ = ctx.solve(cfg)
        assert info.converged and not info.inner_failed
        its = info.iterations
        ctx.set_option("coarse_max_it", 2)
        _x, info, _ = ctx.solve(cfg, raise_on_diverged=False)
        assert info.inner_failed
        ctx.pc_apply_coupled(_ffi.PC_CMG, C.probe_vectors(lv, 29)[0][1])      # stops short too, outside any solve
        ctx.set_option("coarse_max_it", 500)
        _x, info, _ = ctx.solve(cfg)
        assert info.converged and not info.inner_failed and info.iterations == its
        if not on_device:
            _check_cycle(ctx, lv, "host-driven coarsest solve on a small level", smooths=(2,))


# ---- 5. solves ---------------------------------------------------------------------------------------------------------
def _g(field):
    if field == 0:
        return lambda X: np.exp(X[:, 0]) * np.sin(3 * X[:, 1]) + X[:, -1]
    return lambda X: np.cos(2 * X[:, 0]) + X[:, 1] ** 2 - 0.5 * X[:, -1]


@pytest.mark.parametrize("beta", [1.0, 1e2, 1e4])
@pytest.mark.parametrize("name,kind,N", [("quad16", C.QUAD, 16), ("hex8", C.HEX, 8)])
def test_solves_through_solve_dpp(name, kind, N, beta):
    dim = R.dim_of(kind)
    nz = N if dim == 3 else 0
    params = pa.DPPParameters(k1=K1, k2=K2, beta=beta, mu=MU)
    om = o.build_mesh(dim, kind, N, N, nz)
    osys = o.build_system(om, o.Params(k1=K1, k2=K2, beta=beta, mu=MU), _g(0)(om.coords), _g(1)(om.coords), mms=False)
    ud = o.solve_direct(osys)
    lv = _levels(kind, N, N, nz, beta)
    assert abs(lv[0].A - osys.A).max() <= 1e-14 * abs(osys.A).max()
    _x, want, conv = C.cg_count(lv, osys.rhs)
    assert conv
    its = {}
    for label, opts in (("cg", spar.CG_CMG_PARAMS), ("gmres", spar.GMRES_CMG_PARAMS)):
        mesh = fd.UnitSquareMesh(N, N, quadrilateral=True) if dim == 2 else fd.UnitCubeMesh(N, N, N, hexahedral=True, comm=fd.COMM_SELF)
        V = fd.FunctionSpace(mesh, "CG", 1)
        W = V * V
        sol = pa.solve_dpp(W, params, [fd.DirichletBC(W.sub(i), _g(i)) for i in range(2)], solver_parameters=opts)
        x = np.concatenate([np.asarray(f.vector()) for f in sol.solution.subfunctions])
        err = abs(x - ud).max() / abs(ud).max()
        its[label] = sol.iteration_number
        print(f"{name} beta {beta:g} {label}: {sol.iteration_number} iterations (restatement CG {want}), |x - direct| / |direct| = {err:.2e}")
        assert sol.info["converged"] and not sol.info["inner_failed"]
        assert err <= 1e-7
    assert abs(its["cg"] - want) <= 1
    assert its["gmres"] <= its["cg"] + 2


def test_manufactured_solution_errors():
    """quad 32 x 32, the manufactured solution: the L2 errors of CG + coupled MG equal those of GMRES + field-split LU to 1e-8
    (absolute).  Both presets run at ksp_rtol 1e-12 here: the default parameters give pressures of the order 5e3 and 5e5 and L2
    errors of 39.27 and 3 926.5, and at the presets' own rtol 1e-8 the COMPARISON solve is 4.0e-4 off its converged e1_L2
    (39.264648 against 39.265045, where CG + coupled MG at rtol 1e-8 has 39.2650444) - no solver can equal it to 1e-8 there.
    Measured at 1e-12: differences of 1.9e-10 (e1_L2) and 1.1e-9 (e2_L2); the figures at rtol 1e-8 are printed."""
    params = pa.DPPParameters()
    presets = (("cmg", spar.CG_CMG_PARAMS), ("fs-lu", {**spar.GMRES_PARAMS, **spar.FIELDSPLIT_LU_PARAMS}))
    for rtol in (1e-8, 1e-12):
        rows = {}
        for label, opts in presets:
            rows[label] = c2.run_one(N=32, solver=c2.SolverSpec(label, {**opts, "ksp_rtol": rtol, "ksp_atol": 1e-50}), quad=True,
                                     degree=1, params=params)
        for key in ("e1_L2", "e2_L2"):
            print(f"ksp_rtol {rtol:g} {key}: cmg {rows['cmg'][key]!r} ({rows['cmg']['it']} its) against fs-lu {rows['fs-lu'][key]!r} "
                  f"({rows['fs-lu']['it']} its), difference {abs(rows['cmg'][key] - rows['fs-lu'][key]):.3e}")
    for key in ("e1_L2", "e2_L2"):
        assert abs(rows["cmg"][key] - rows["fs-lu"][key]) <= 1e-8
    assert rows["cmg"]["it"] <= 20


# ---- 6. condition numbers -------------------------------------------------------------------------------------------------
def test_condition_numbers():
    N = 16
    params = pa.DPPParameters(k1=K1, k2=K2, beta=1e2, mu=MU)
    lv = _levels(C.QUAD, N, N, 0, 1e2)
    ev, _B = C.ba_spectrum(lv, 2)
    want = ev.max() / ev.min()
    mesh = pa.create_mesh(N, N, quadrilateral=True)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    bcs = [fd.DirichletBC(W.sub(0), fd.Constant(0.0), "on_boundary"), fd.DirichletBC(W.sub(1), fd.Constant(0.0), "on_boundary")]
    a, _ = pa.dpp_form(W, params)
    got = conditioning.preconditioned_condition_number(a, bcs, "pph_cmg")
    eff = conditioning.effective_condition_numbers(W, params, bcs, spar.CG_CMG_PARAMS)
    print(f"kappa(B A): device {got:.6f}, dense eig of the restatement {want:.6f}, effective {eff}")
    assert abs(got - want) <= 1e-3 * want
    assert set(eff) == {"monolithic"} and abs(eff["monolithic"] - want) <= 1e-3 * want
    # mg_smooth is honoured
    ev3, _B = C.ba_spectrum(lv, 3)
    got3 = conditioning.preconditioned_condition_number(a, bcs, "pph_cmg", mg_smooth=3)
    assert abs(got3 - ev3.max() / ev3.min()) <= 1e-3 * got3


# ---- 7. refusals at the C level --------------------------------------------------------------------------------------------
def _cfg(**kw):
    cfg, _ = translate_options(spar.CG_CMG_PARAMS)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_refusals_leave_the_context_usable():
    kind, nx, ny, nz = MESHES["quad16x12"]
    lv = _levels(kind, nx, ny, nz, 1e2)
    with _open(kind, nx, ny, nz) as ctx:
        nodes = _nodes(kind, nx, ny, nz, "boundary")
        for f in (0, 1):
            ctx.set_dirichlet(f, nodes[f], R.dirichlet_values(kind, nx, ny, nz, nodes[f], f))
        # without the monolithic assembly
        ctx.assemble(K1, K2, 1e2, MU, monolithic=False)
        with pytest.raises(ValueError, match="monolithic"):
            ctx.solve(_cfg())
        with pytest.raises(ValueError, match="monolithic"):
            ctx.pc_apply_coupled(_ffi.PC_CMG, np.ones(2 * ctx.n))
        ctx.assemble(K1, K2, 1e2, MU, monolithic=True)
        # as a block preconditioner, with Picard sweeps
        fs, _ = translate_options(spar.FIELDSPLIT_MG_PARAMS)
        fs.inner_pc_type = _ffi.PC_CMG
        with pytest.raises(ValueError, match="pph_cmg"):
            ctx.solve(fs)
        pic, _ = translate_options(spar.PICARD_MG_SOLVER_PARAMS, nonlinear=True)
        pic.inner_pc_type = _ffi.PC_CMG
        with pytest.raises(ValueError, match="pph_cmg"):
            ctx.solve(pic)
        with pytest.raises(ValueError, match="pph_cmg"):
            ctx.solve(_cfg(picard=1))
        with pytest.raises(ValueError):
            ctx.pc_apply(0, _ffi.PC_CMG, np.ones(ctx.n))
        with pytest.raises(ValueError):
            ctx.pc_apply_coupled(_ffi.PC_MG, np.ones(2 * ctx.n))
        with pytest.raises(ValueError):
            ctx.preconditioned_extremes(_ffi.MAT_A11, _ffi.PC_CMG)
        # the scalar cycle on the monolithic operator stays refused
        with pytest.raises(ValueError):
            ctx.solve(_cfg(pc_type=_ffi.PC_MG))
        # ... and the context still works
        _check_cycle(ctx, lv, "after the refusals", smooths=(2,))
        x, info, _ = ctx.solve(_cfg())
        assert info.converged
        # the other monolithic preconditioners of the entry point
        A = lv[0].A
        r = C.probe_vectors(lv, 23)[0][1]
        zj = ctx.pc_apply_coupled(_ffi.PC_JACOBI, r)
        assert C.rel_err(zj, r / A.diagonal()) <= 1e-13
        zb = ctx.pc_apply_coupled(_ffi.PC_BLOCK2, r)
        assert C.rel_err(zb, o.block2_jacobi_apply(A, lv[0].n)(r)) <= 1e-12
    # a degree-2 context
    with _ffi.Context(0) as ctx2:
        ctx2.mesh_build_lagrange(2, _ffi.CELL_QUAD, 4, 4, 0, degree=2)
        for f in (0, 1):
            ctx2.set_dirichlet(f, np.array([0, 5], np.int64), np.array([1.0, -2.0 - f]))
        ctx2.assemble(K1, K2, 1.0, MU, monolithic=True)
        with pytest.raises(ValueError, match="degree-2"):
            ctx2.solve(_cfg())
        with pytest.raises(ValueError, match="degree-2"):
            ctx2.pc_apply_coupled(_ffi.PC_CMG, np.ones(2 * ctx2.n))
        cfg, _ = translate_options({**spar.GMRES_ILU_PARAMS, "ksp_max_it": 500})
        _x, info, _ = ctx2.solve(cfg, raise_on_diverged=False)
        assert info.converged and info.iterations > 0
