"""Option `presmooth_lazy`: a CG update that the host expects to be the last of its block solve does not write the next
multigrid cycle's pre-smoothed first guess; a cycle that runs after all forms it itself (`k_cheb_init`: the same expression
in the same order).  Results must be bit for bit what they are with every update writing the guess.

Every case builds one context, assembles once and solves with `presmooth_lazy` 0, then 1 (and 2, the iteration-count
rule): the full solution, the counts, the norms and the residual history must be EQUAL, not close.  The counters of
`Context.timers()` say which route ran:

* `presmooth_skipped` updates launched without the guess, `presmooth_late` cycles that then started with `k_cheb_init`,
  `presmooth_unused` updates that wrote a guess no cycle read.

Meshes.  hex 16^3 and quad 40 x 36 have a hierarchy whose fine level is swept by the full-chip kernels (the route in
question).  hex 20 x 18 x 15 cannot be coarsened (15 cells): its preconditioner is the single-level Chebyshev polynomial, no
CG update writes a guess there, so the case pins equality and counters of 0; hex 20 x 18 x 16 (node lines of 21, 19 and 17:
odd lengths, partial last chunks, two levels) is the ragged mesh on which the route does run and the counters are asserted.

The slab path (merged all-reduce) takes the same decision from numbers that are equal on all ranks; it has no 0-against-1
comparison of its own here - the two-rank comparisons of test_gpu_multirank.py against a single context run with the option on.

Each case prints its counters; `-s` shows them."""
import numpy as np
import pytest

from oracle import dpp_oracle as o

pytestmark = pytest.mark.gpu

K2 = 1e-2


def _ctx(make, dim, kind, nx, ny, nz=0, k2=K2, monolithic=False, **options):
    from perphil_amd import _ffi

    p = o.Params(k1=1.0, k2=k2, beta=1.0, mu=1.0)
    om = o.build_mesh(dim, {"hex": o.CELL_HEX, "quad": o.CELL_QUAD, "tet": o.CELL_TET}[kind], nx, ny, nz)
    ctx = make()
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.mesh_build(dim, {"hex": _ffi.CELL_HEX, "quad": _ffi.CELL_QUAD, "tet": _ffi.CELL_TET}[kind], nx, ny, nz)
    b = o.boundary_nodes(om)
    e1, e2 = o.exact_pressures(om.coords, p)
    ctx.set_dirichlet(0, b, e1[b])
    ctx.set_dirichlet(1, b, e2[b])
    ctx.assemble(p.k1, p.k2, p.beta, p.mu, monolithic=monolithic)
    return ctx


def _picard_cfg(inner_reduction=1e-1, inner_rtol=1e-10, inner_norm=1, inner_max_it=50000):
    """The benchmark's Picard configuration (bench.py picard_cfg with its defaults: mg_smooth 1)."""
    from perphil_amd import _ffi

    cfg = _ffi.SolverCfg()
    cfg.ksp_type, cfg.pc_type, cfg.restart, cfg.max_it = _ffi.KSP_GMRES, _ffi.PC_FIELDSPLIT, 30, 50000
    cfg.rtol, cfg.atol = 1e-8, 1e-12
    cfg.inner_ksp_type, cfg.inner_pc_type, cfg.inner_max_it = _ffi.KSP_CG, _ffi.PC_MG, inner_max_it
    cfg.inner_rtol, cfg.inner_atol = inner_rtol, 1e-300
    cfg.picard, cfg.picard_rtol, cfg.picard_atol, cfg.picard_max_it = 1, 1e-8, 1e-12, 100
    cfg.mg_smooth, cfg.inner_reduction, cfg.inner_norm = 1, inner_reduction, inner_norm
    return cfg


def _fieldsplit_cfg(inner_norm):
    """bench.py config5_cfg: GMRES(30) + multiplicative field-split, cold CG + multigrid block solves to 1e-10."""
    from perphil_amd import _ffi

    cfg = _ffi.SolverCfg()
    cfg.ksp_type, cfg.pc_type, cfg.restart, cfg.max_it, cfg.rtol, cfg.atol = _ffi.KSP_GMRES, _ffi.PC_FIELDSPLIT, 30, 200, 1e-8, 1e-12
    cfg.inner_ksp_type, cfg.inner_pc_type, cfg.inner_max_it, cfg.inner_rtol, cfg.inner_atol = _ffi.KSP_CG, _ffi.PC_MG, 500, 1e-10, 1e-300
    cfg.picard, cfg.picard_rtol, cfg.picard_atol, cfg.picard_max_it, cfg.mg_smooth = 0, 1e-8, 1e-12, 100, 1
    cfg.inner_reduction, cfg.inner_norm = 0.0, inner_norm
    return cfg


def _solve(ctx, cfg, lazy):
    ctx.set_option("presmooth_lazy", lazy)
    x, info, hist = ctx.solve(cfg, hist_cap=256)
    t = ctx.timers()
    rec = (int(info.iterations), int(info.inner_iterations), float(info.resnorm), float(info.rhs_norm), int(info.converged),
           int(info.inner_failed))
    return x.copy(), rec, hist.copy(), {k: t[k] for k in ("presmooth_skipped", "presmooth_late", "presmooth_unused")}


def _both_ways(tag, ctx, cfg):
    """Solves with the option 0, 1 and 2; asserts bitwise equality; returns the counters of the three runs."""
    x0, rec0, hist0, c0 = _solve(ctx, cfg, 0)
    assert rec0[4] == 1 and rec0[5] == 0
    assert (c0["presmooth_skipped"], c0["presmooth_late"]) == (0, 0)
    out = [c0]
    for lazy in (1, 2):
        x, rec, hist, c = _solve(ctx, cfg, lazy)
        print(f"{tag}: presmooth_lazy {lazy}: sweeps/its {rec[0]}, inner {rec[1]}, counters {c} (option 0: {c0})")
        assert np.array_equal(x, x0)
        assert rec == rec0
        assert np.array_equal(hist, hist0)
        # the last update of every solve either wrote a guess nobody read or was launched without one and not followed by
        # a cycle; with the option off it is always the former
        assert c["presmooth_unused"] + c["presmooth_skipped"] - c["presmooth_late"] == c0["presmooth_unused"]
        out.append(c)
    return out


HIERARCHY = [("hex", 3, 16, 16, 16), ("hex", 3, 20, 18, 16), ("quad", 2, 40, 36, 0)]
ID_H = ["hex16", "hex20x18x16", "quad40x36"]


@pytest.mark.parametrize("kind,dim,nx,ny,nz", HIERARCHY, ids=ID_H)
def test_inexact_picard_skips_and_stays_bitwise(gpu_ctx_factory, kind, dim, nx, ny, nz):
    """inner_reduction 1e-1, unpreconditioned norm: most block solves take one iteration - their update needs no guess."""
    ctx = _ctx(gpu_ctx_factory, dim, kind, nx, ny, nz)
    c0, c1, c2 = _both_ways(f"{kind} {nx}x{ny}x{nz} inexact", ctx, _picard_cfg())
    assert c0["presmooth_unused"] > 0            # what the option is for: guesses written for nothing
    assert c1["presmooth_skipped"] > 0
    assert c1["presmooth_unused"] < c0["presmooth_unused"]


@pytest.mark.parametrize("kind,dim,nx,ny,nz,k2", [("hex", 3, 16, 16, 16, 1e-2), ("hex", 3, 20, 18, 16, 1e-4), ("quad", 2, 40, 36, 0, 1e-2)],
                         ids=["hex16", "hex20x18x16-k2=1e-4", "quad40x36"])
def test_many_iteration_solves_take_the_late_route(gpu_ctx_factory, kind, dim, nx, ny, nz, k2):
    """inner_reduction 0, inner_rtol 1e-10: block solves of several iterations, whose contraction varies - a solve that
    goes on after an update launched without the guess must start its next cycle with k_cheb_init.  With k2 = 1e-2 the
    residual rule reaches that route on hex 16^3 and quad 40 x 36; on hex 20 x 18 x 16 every prediction holds with that
    k2, so the ragged mesh runs with k2 = 1e-4, where one does not."""
    ctx = _ctx(gpu_ctx_factory, dim, kind, nx, ny, nz, k2=k2)
    c0, c1, c2 = _both_ways(f"{kind} {nx}x{ny}x{nz} k2 {k2} rtol 1e-10", ctx, _picard_cfg(inner_reduction=0.0))
    assert c1["presmooth_late"] >= 1
    for c in (c1, c2):
        assert c["presmooth_late"] <= c["presmooth_skipped"]


def test_mesh_without_hierarchy_is_untouched(gpu_ctx_factory):
    """hex 20 x 18 x 15: no coarser level, no fused cycle, so no update ever wrote a guess: equal results, counters 0."""
    ctx = _ctx(gpu_ctx_factory, 3, "hex", 20, 18, 15)
    for cfg in (_picard_cfg(), _picard_cfg(inner_reduction=0.0)):
        for c in _both_ways("hex 20x18x15", ctx, cfg):
            assert (c["presmooth_skipped"], c["presmooth_late"], c["presmooth_unused"]) == (0, 0, 0)


def test_iteration_limit_is_a_certain_last_update(gpu_ctx_factory):
    """inner_max_it 2 with an unreachable tolerance: the second update of every solve is its last for certain, the first
    one is followed by a cycle.  The block solves end unconverged (reported), identically both ways."""
    ctx = _ctx(gpu_ctx_factory, 3, "hex", 16, 16, 16)
    cfg = _picard_cfg(inner_reduction=0.0, inner_rtol=1e-30, inner_max_it=2)
    cfg.picard_max_it = 3
    res = []
    for lazy in (0, 1):
        ctx.set_option("presmooth_lazy", lazy)
        x, info, hist = ctx.solve(cfg, hist_cap=16, raise_on_diverged=False)
        res.append((x.copy(), int(info.iterations), int(info.inner_iterations), float(info.resnorm), hist.copy(), ctx.timers()))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1:4] == res[1][1:4] and np.array_equal(res[0][4], res[1][4])
    assert res[0][2] == 12                                        # 3 sweeps x 2 blocks x 2 iterations
    t = res[1][5]
    assert (t["presmooth_skipped"], t["presmooth_late"], t["presmooth_unused"]) == (6, 0, 0)


@pytest.mark.parametrize("inner_norm", [0, 1])
def test_fieldsplit_gmres_cold_block_solves(gpu_ctx_factory, inner_norm):
    """tet 8^3, GMRES + multiplicative field-split: cold block solves whose counts repeat from application to application.
    inner_norm 0 is bench.py's config 5 (preconditioned-norm CG: not the loop in question, counters 0); inner_norm 1 sends
    the same solves through the unpreconditioned-norm loop."""
    ctx = _ctx(gpu_ctx_factory, 3, "tet", 8, 8, 8, k2=1e-4, monolithic=True)
    c0, c1, c2 = _both_ways(f"tet 8^3 field-split inner_norm {inner_norm}", ctx, _fieldsplit_cfg(inner_norm))
    if inner_norm == 0:
        for c in (c0, c1, c2):
            assert (c["presmooth_skipped"], c["presmooth_late"], c["presmooth_unused"]) == (0, 0, 0)
    else:
        assert c0["presmooth_unused"] > 0 and c2["presmooth_skipped"] > 0


def test_fixed_iteration_solves_do_not_count(gpu_ctx_factory):
    """inner_norm 2 (cg_solve_fixed: the host knows the last update, which never wrote a guess): equal, counters 0."""
    ctx = _ctx(gpu_ctx_factory, 3, "hex", 16, 16, 16)
    for c in _both_ways("hex 16^3 inner_norm 2", ctx, _picard_cfg(inner_norm=2, inner_max_it=2)):
        assert (c["presmooth_skipped"], c["presmooth_late"], c["presmooth_unused"]) == (0, 0, 0)


def test_replayed_iteration_bodies_stay_bitwise(gpu_ctx_factory):
    """use_graphs 2: iteration bodies are replayed with fixed arguments, so nothing is skipped there."""
    ctx = _ctx(gpu_ctx_factory, 3, "hex", 16, 16, 16)
    ctx.set_option("use_graphs", 2)
    for cfg in (_picard_cfg(), _picard_cfg(inner_reduction=0.0)):
        c0, c1, c2 = _both_ways("hex 16^3 use_graphs 2", ctx, cfg)
        assert c1["presmooth_skipped"] == 0 and c2["presmooth_skipped"] == 0
