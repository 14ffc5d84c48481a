"""p-multigrid (block pc_type pph_pmg) on the device: the cycle itself against the NumPy restatement
(tests/pmg_restatement.py) through pph_pc_apply, the block solves and whole solves built on it, hierarchy refresh,
degree-1 identity with mg, and the degree-2 convergence study with the multigrid solvers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import p2_restatement as R  # noqa: E402
import pmg_restatement as PM  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

import perphil_amd as pa  # noqa: E402
from perphil_amd import _ffi, convergence_2d as c2, fd, solver_parameters as spar  # noqa: E402
from perphil_amd.solver import translate_options  # noqa: E402

pytestmark = pytest.mark.gpu

K1, K2, BETA, MU = 1.0, 0.01, 1.0, 1.0
# odd / non-cubic meshes (the CG-1 part cannot be coarsened) and coarsenable ones, all four kinds
MESHES = {
    "quad5x3": (R.QUAD, 5, 3, 0), "tri5x3": (R.TRI, 5, 3, 0), "hex3x4x2": (R.HEX, 3, 4, 2), "tet3x4x2": (R.TET, 3, 4, 2),
    "quad8x8": (R.QUAD, 8, 8, 0), "tri16x8": (R.TRI, 16, 8, 0), "hex8x8x4": (R.HEX, 8, 8, 4), "tet8x8x4": (R.TET, 8, 8, 4),
}
COEF_K = (K1 / MU, K2 / MU)


def _data(kind, nx, ny, nz, variant=0):
    """Dirichlet nodes and non-zero data; variant 1: another set (three faces / sides only) with other values."""
    X = R.coords(kind, nx, ny, nz)
    b = R.boundary_nodes(kind, nx, ny, nz)
    if variant == 1:
        b = b[X[b, 0] < 1.0 - 1e-12]          # the side x = 1 becomes a natural boundary
        return b, 1.0 + X[b, 1] ** 2, np.cos(X[b, 0]) - X[b, -1]
    return b, np.exp(X[b, 0]) * np.sin(3 * X[b, 1]), np.cos(2 * X[b, 0]) + X[b, -1]


def _setup(ctx, kind, nx, ny, nz, k1=K1, k2=K2, variant=0, monolithic=True):
    b, g1, g2 = _data(kind, nx, ny, nz, variant)
    ctx.set_dirichlet(0, b, g1)
    ctx.set_dirichlet(1, b, g2)
    ctx.assemble(k1, k2, BETA, MU, monolithic=monolithic)
    mask = np.zeros(ctx.n, bool)
    mask[b] = True
    return b, g1, g2, mask


def _new_ctx(gpu_ctx_factory, kind, nx, ny, nz, degree=2):
    ctx = gpu_ctx_factory()
    ctx.mesh_build_lagrange(R.dim_of(kind), kind, nx, ny, nz, degree)
    return ctx


def _check_cycle(ctx, kind, nx, ny, nz, mask, k1, k2, seed):
    rng = np.random.default_rng(seed)
    for which, ck in ((0, k1 / MU), (1, k2 / MU)):
        lv = PM.build_levels(kind, nx, ny, nz, ck, BETA / MU, mask)
        for ns in (1, 2):
            r = rng.standard_normal(ctx.n)
            rm = r.copy()
            rm[mask] = 0.0
            ref = PM.cycle(lv, rm, ns)
            ctx.set_option("pmg_fused", 1)
            z = ctx.pc_apply(which, _ffi.PC_PMG, r, mg_smooth=ns)
            err = abs(z - ref).max() / abs(ref).max()
            print(f"kind {kind} {nx}x{ny}x{nz} block {which} mg_smooth {ns}: |z - ref| / |ref| = {err:.3e}")
            assert err <= 1e-10
            assert not z[mask].any()                                   # exactly 0 on constrained entries
            assert np.array_equal(z, ctx.pc_apply(which, _ffi.PC_PMG, r, mg_smooth=ns))   # bitwise reproducible
            ctx.set_option("pmg_fused", 0)
            zg = ctx.pc_apply(which, _ffi.PC_PMG, r, mg_smooth=ns)
            ctx.set_option("pmg_fused", 1)
            assert abs(z - zg).max() <= 1e-12 * abs(zg).max()
            assert abs(zg - ref).max() <= 1e-10 * abs(ref).max()


@pytest.mark.parametrize("name", list(MESHES))
def test_cycle_against_restatement(gpu_ctx_factory, name):
    kind, nx, ny, nz = MESHES[name]
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    _, _, _, mask = _setup(ctx, kind, nx, ny, nz)
    _check_cycle(ctx, kind, nx, ny, nz, mask, K1, K2, seed=11)


def _restated_block_counts(kind, nx, ny, nz, b, g1, g2, mask, k1, k2, rtol):
    """CG iterations of Picard's first sweep (cold block solves, zero guess) with the restated cycle."""
    Kr, Mr = R.assemble_KM(kind, nx, ny, nz)
    A11, A22, A12, A21, rhs, u0 = R.eliminate(Kr, Mr, b, g1, g2, k1, k2, BETA, MU)
    n = mask.size
    lv1 = PM.build_levels(kind, nx, ny, nz, k1 / MU, BETA / MU, mask)
    lv2 = PM.build_levels(kind, nx, ny, nz, k2 / MU, BETA / MU, mask)
    r1 = o.pcg(A11.tocsr(), rhs[:n], lambda v: PM.cycle(lv1, v, 2), rtol=rtol, atol=1e-50, max_it=500)
    r2 = o.pcg(A22.tocsr(), rhs[n:] - A21 @ r1.x, lambda v: PM.cycle(lv2, v, 2), rtol=rtol, atol=1e-50, max_it=500)
    return r1.its, r2.its


def _check_solves(ctx, kind, nx, ny, nz, b, g1, g2, mask, k1, k2):
    """Field-split GMRES and Picard with pph_pmg block solves against GMRES + ILU(0) on the same context."""
    cfg_ilu, _ = translate_options({**spar.GMRES_ILU_PARAMS, "ksp_rtol": 1e-12, "ksp_atol": 1e-30})
    x_ilu, info, _ = ctx.solve(cfg_ilu)
    assert info.converged
    x_ilu = x_ilu.copy()
    scale = abs(x_ilu).max()
    for label, opts, nonlinear, tol in [("fieldsplit", spar.FIELDSPLIT_PMG_PARAMS, False, 1e-8),
                                        ("picard", spar.PICARD_PMG_SOLVER_PARAMS, True, 1e-8)]:
        cfg, _ = translate_options(opts, nonlinear=nonlinear)
        assert cfg.inner_pc_type == _ffi.PC_PMG
        x, info, _ = ctx.solve(cfg)
        err = abs(x - x_ilu).max() / scale
        print(f"kind {kind} {nx}x{ny}x{nz} {label}: outer {info.iterations}, inner CG {info.inner_iterations}, "
              f"|x - x_ilu| / |x_ilu| = {err:.3e}")      # whole-solve counts: recorded, the oracle restates neither loop with a pluggable block pc
        assert info.converged and not info.inner_failed
        assert err <= 10 * tol
    # one Picard sweep = two cold block solves: exactly the restatement's CG iterations
    cfg, _ = translate_options({**spar.PICARD_PMG_SOLVER_PARAMS, "snes_max_it": 1}, nonlinear=True)
    _, info, _ = ctx.solve(cfg, raise_on_diverged=False)
    want = _restated_block_counts(kind, nx, ny, nz, b, g1, g2, mask, k1, k2, rtol=cfg.inner_rtol)
    print(f"kind {kind} {nx}x{ny}x{nz} first sweep: device {info.inner_iterations}, restatement {want}")
    assert info.iterations == 1 and info.inner_iterations == sum(want)
    return want


@pytest.mark.parametrize("name", list(MESHES))
def test_block_solves_and_whole_solves(gpu_ctx_factory, name):
    kind, nx, ny, nz = MESHES[name]
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    b, g1, g2, mask = _setup(ctx, kind, nx, ny, nz)
    _check_solves(ctx, kind, nx, ny, nz, b, g1, g2, mask, K1, K2)


@pytest.mark.parametrize("name", ["quad8x8", "tet8x8x4"])
def test_through_solve_dpp(name):
    """The presets through solve_dpp / solve_dpp_nonlinear: the GMRES + ILU(0) solution to 10x the outer tolerance."""
    kind, nx, ny, nz = MESHES[name]
    params = pa.DPPParameters(k1=K1, k2=K2, beta=BETA, mu=MU)

    def g(X):
        return np.exp(X[:, 0]) * np.sin(3 * X[:, 1]) + X[:, -1]

    def run(solve, opts):
        mesh = (fd.UnitSquareMesh(nx, ny, quadrilateral=(kind == R.QUAD)) if R.dim_of(kind) == 2
                else fd.UnitCubeMesh(nx, ny, nz, hexahedral=(kind == R.HEX), comm=fd.COMM_SELF))
        V = fd.FunctionSpace(mesh, "CG", 2)
        W = V * V
        sol = solve(W, params, [fd.DirichletBC(W.sub(i), g) for i in range(2)], solver_parameters=opts)
        return sol, np.concatenate([np.asarray(f.vector()) for f in sol.solution.subfunctions])

    _, x_ilu = run(pa.solve_dpp, {**spar.GMRES_ILU_PARAMS, "ksp_rtol": 1e-12, "ksp_atol": 1e-30})
    for solve, opts in [(pa.solve_dpp, spar.FIELDSPLIT_PMG_PARAMS), (pa.solve_dpp_nonlinear, spar.PICARD_PMG_SOLVER_PARAMS)]:
        sol, x = run(solve, opts)
        assert sol.info["converged"] and not sol.info["inner_failed"]
        assert abs(x - x_ilu).max() <= 10 * 1e-8 * abs(x_ilu).max()


@pytest.mark.parametrize("name,sizes", [("quad", (16, 32, 64)), ("tri", (16, 32, 64)), ("hex", (8, 16)), ("tet", (8, 16))])
def test_mesh_independence(gpu_ctx_factory, name, sizes):
    """Inner CG counts of the first Picard sweep do not grow with the mesh (cap 2: the restatement stays within 1)."""
    kind = {"quad": R.QUAD, "tri": R.TRI, "hex": R.HEX, "tet": R.TET}[name]
    counts = []
    for N in sizes:
        nz = N if R.dim_of(kind) == 3 else 0
        ctx = _new_ctx(gpu_ctx_factory, kind, N, N, nz)
        _setup(ctx, kind, N, N, nz, monolithic=False)
        cfg, _ = translate_options({**spar.PICARD_PMG_SOLVER_PARAMS, "snes_max_it": 1}, nonlinear=True)
        _, info, _ = ctx.solve(cfg, raise_on_diverged=False)
        assert not info.inner_failed
        counts.append(int(info.inner_iterations))
        ctx.close()
    print(name, sizes, "inner CG iterations of the first sweep (both blocks):", counts)
    assert max(counts) - min(counts) <= 2


def test_hierarchy_refresh(gpu_ctx_factory):
    """Re-assembly with other parameters, then a changed Dirichlet set: the hierarchy follows both."""
    kind, nx, ny, nz = MESHES["hex8x8x4"]
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    b, g1, g2, mask = _setup(ctx, kind, nx, ny, nz)
    _check_cycle(ctx, kind, nx, ny, nz, mask, K1, K2, seed=5)
    k1, k2 = 0.3, 2.0
    b, g1, g2, mask = _setup(ctx, kind, nx, ny, nz, k1=k1, k2=k2)
    _check_cycle(ctx, kind, nx, ny, nz, mask, k1, k2, seed=6)
    b, g1, g2, mask = _setup(ctx, kind, nx, ny, nz, k1=k1, k2=k2, variant=1)
    _check_cycle(ctx, kind, nx, ny, nz, mask, k1, k2, seed=7)
    _check_solves(ctx, kind, nx, ny, nz, b, g1, g2, mask, k1, k2)


@pytest.mark.parametrize("name", ["quad8x8", "tet8x8x4", "quad5x3"])
def test_degree1_pmg_is_mg(gpu_ctx_factory, name):
    kind, nx, ny, nz = MESHES[name]
    res = {}
    for pc, mgopts, pmgopts in [("fs", spar.FIELDSPLIT_MG_PARAMS, spar.FIELDSPLIT_PMG_PARAMS),
                                ("picard", spar.PICARD_MG_SOLVER_PARAMS, spar.PICARD_PMG_SOLVER_PARAMS)]:
        for key, opts in (("mg", mgopts), ("pmg", pmgopts)):
            ctx = gpu_ctx_factory()
            ctx.mesh_build(R.dim_of(kind), kind, nx, ny, nz)
            om = o.build_mesh(R.dim_of(kind), kind, nx, ny, nz)
            bn = o.boundary_nodes(om)
            ctx.set_dirichlet(0, bn, np.sin(om.coords[bn, 0]) + 1.0)
            ctx.set_dirichlet(1, bn, om.coords[bn, 1] ** 2)
            ctx.assemble(K1, K2, BETA, MU, monolithic=True)
            cfg, _ = translate_options(opts, nonlinear=(pc == "picard"))
            x, info, _ = ctx.solve(cfg)
            res[key] = (x.copy(), info.iterations, info.inner_iterations, info.converged)
            if key == "pmg":
                r = np.random.default_rng(2).standard_normal(ctx.n)
                assert np.array_equal(ctx.pc_apply(0, _ffi.PC_PMG, r), ctx.pc_apply(0, _ffi.PC_MG, r))
            ctx.close()
        assert res["mg"][1:] == res["pmg"][1:] and res["mg"][3]
        assert np.array_equal(res["mg"][0], res["pmg"][0])


def test_mg_at_degree2_still_refused(gpu_ctx_factory):
    kind, nx, ny, nz = MESHES["quad8x8"]
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    _setup(ctx, kind, nx, ny, nz)
    for opts, nonlinear in [(spar.FIELDSPLIT_MG_PARAMS, False), (spar.PICARD_MG_SOLVER_PARAMS, True)]:
        cfg, _ = translate_options(opts, nonlinear=nonlinear)
        with pytest.raises(ValueError, match="multigrid"):      # PPH_ERR_INVALID
            ctx.solve(cfg)
    with pytest.raises(ValueError):
        ctx.pc_apply(0, _ffi.PC_MG, np.ones(ctx.n))
    with pytest.raises(ValueError):
        ctx.pc_apply(0, _ffi.PC_FIELDSPLIT, np.ones(ctx.n))
    # the other block preconditioners through the same entry point: Jacobi against the diagonal
    A11 = ctx.csr(_ffi.MAT_A11)
    r = np.random.default_rng(4).standard_normal(ctx.n)
    z = ctx.pc_apply(0, _ffi.PC_JACOBI, r)
    b = _data(kind, nx, ny, nz)[0]
    rm = r.copy()
    rm[b] = 0.0
    assert abs(z - rm / A11.diagonal()).max() <= 1e-14 * abs(z).max()
    zi = ctx.pc_apply(0, _ffi.PC_ILU, r)
    fac = R.ilu0(A11)
    assert abs(zi - R.ilu_apply(fac, rm)).max() <= 1e-10 * abs(zi).max()


def test_convergence_orders_with_pmg():
    """The degree-2 study of tests/test_p2_gpu.py::test_convergence_orders with the p-multigrid solvers: same meshes, same
    fit, same margins; at every N the error norms are those of GMRES + ILU(0) to 1e-6 relative (all solves are run to
    tight residual tolerances, so that what is compared is the discrete solution)."""
    params = pa.DPPParameters()
    ilu = c2.SolverSpec("GMRES + ILU PC", {**spar.GMRES_ILU_PARAMS, "ksp_rtol": 1e-12, "ksp_atol": 1e-30})
    blk = {"ksp_type": "cg", "pc_type": "pph_pmg", "ksp_rtol": 1e-13}
    tight = {"fieldsplit_0": blk, "fieldsplit_1": blk}
    fs, pic = c2.pmg_solvers()
    specs = [c2.SolverSpec(fs.name, {**fs.params, **tight, "ksp_rtol": 1e-12, "ksp_atol": 1e-30}),
             c2.SolverSpec(pic.name, {**pic.params, **tight, "snes_rtol": 1e-12, "snes_atol": 1e-30}, nonlinear=True)]
    for quad in (True, False):
        base = {N: c2.run_one(N, ilu, quad=quad, degree=2, params=params) for N in (8, 16, 32, 64)}
        for spec in specs:
            rows = [c2.run_one(N, spec, quad=quad, degree=2, params=params) for N in (8, 16, 32, 64)]
            for r in rows:
                for e in c2.ERROR_FIELDS:
                    rel = abs(r[e] - base[r["N"]][e]) / base[r["N"]][e]
                    print(f"quad {quad} {spec.name} N {r['N']} it {r['it']} {e} {r[e]:.6e} rel. to ILU {rel:.2e}")
                    assert rel <= 1e-6, (quad, spec.name, r["N"], e)
            slopes = {r["err"]: r["slope"] for r in c2.observed_orders(rows[1:])}
            for e in ("e1_L2", "e2_L2"):
                assert abs(slopes[e] - 3.0) <= 0.2, (quad, spec.name, e, slopes)
            for e in ("e1_H1s", "e2_H1s"):
                assert abs(slopes[e] - 2.0) <= 0.2, (quad, spec.name, e, slopes)
