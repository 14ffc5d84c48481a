"""The monolithic Krylov loops of perphil_amd/csrc/pph_solve.hip (cg_solve with the preconditioned norm, gmres_solve) and the
BLAS-1 kernels of pph_la.hip they run on, past the vector kernels' launch caps, against the restated loops of
tests/krylov_reference.py.

A Krylov loop repairs its own arithmetic: a reduction or an update that loses the ragged tail of its last grid-stride pass still
converges, a few iterations later.  So nothing here waits for convergence.  Every run is ctx.solve_rhs with rtol = atol = 0 and a
small max_it - the k-th iterate and hist[0 .. k] - held entry by entry against the same loop in NumPy fp64:

  quad 1024x512   N = 1 051 650: a third pass of 3 074 rows in every 2n-long kernel (ew_grid: 2048 x 256 threads, two entries each),
                  1024 partial sums per reduction slot in five passes, a second pass of 1 537 nodes in k_block2_build.  GMRES restart
                  7, max_it 10 (multi-dot widths 1, 2, 2+1, 4, 4+1, 4+2, 4+2+1; one restart; a second cycle cut after 3 columns)
                  and CG max_it 6, each with pc none / jacobi / pph_block2
  quad 2048x512   n = 1 051 137: a third pass of 2 561 nodes in k_block2 (it loops over n, not 2n); CG and GMRES with pph_block2
  hex 128x64x64   N = 1 090 050: rows of up to 54 entries in k_spmv_wide<8, DOT> (two 4-wide steps of 8 lanes) on a grid of 1024
                  workgroups for 34 065 chunks of 32 rows, with the fused p.Ap; CG with jacobi

and on quad 1024x512 the option sets fetch_spin 0, spmv_lanes 16, spmv_blocks 2048 (2048 partial sums into one slot) and
l3_order_min_rows 1000 (k_set, k_copy, k_sub descending: bit-identical to the default run).  Every case asserts from
krylov_reference.la_launch / block2_launch / spmv_launch which side of its cap it is on.

Mesh, Dirichlet sets and data are those of asm_scale_reference (CF, unshifted); b is seeded uniform in [0.5, 1.5].

Bound.  Nothing is taken from the device.  delta_hist (relative, per entry) and delta_x (max |dx| / max |x|) are the larger of
the discrepancies of the fp64 restatement against its longdouble run and against its run on the `perturbed` system (every
product times 1 + 4 eps xi row by row).  The device must stay within max(100 delta, 1e-13) of the fp64 restatement - the rule of
tests/README.md for the norms.  info.iterations, info.converged and info.resnorm == hist[-1] are exact.  Every case prints its worst
fraction of the bar before it asserts.  The host file (tests/test_krylov_scale_host.py) shows that leaving the last pass out of any
one vector kernel misses these bars by a factor of 1e7 or more.

The longdouble run is longdouble THROUGHOUT (krylov_reference.LongdoubleSystem): box matrices included.  A longdouble run that
reads the fp64-rounded box matrices of the fp64 run has, to the last bit, the fp64 run's operator, and delta then holds the rounding
of the loop's sums and products only (7e-16 for Jacobi-CG on quad 1024x512).  But the device does not hold that operator: it holds
assembled entries, each an fp64 rounding of its own, and two fp64 roundings of one operator differ by half an ulp per entry in the
SAME way in every product and relative to |A| |x|, which a stiffness row cancels by 1 / h^2 on the smooth part of a vector.  With
the first form of the longdouble run Jacobi-CG and block2-CG on quad 1024x512 were 3.5e-13 from the matrix-free restatement on the
device - and the same loop on the host's own fp64 CSR 1.8e-13 (host file, no device) - against a delta of 7e-16.  With box
matrices in longdouble the fp64 restatement is itself 6.2e-14 from its longdouble run there: that is the reference's own
error, and the bar is 100 times it as before.

Two references.  Every large case, option set and small mesh runs twice: against the matrix-free restatement under that bar,
and against the same restated loop on the matrix the context assembled (exported CSR).  There both sides hold one stored
operator, and the bar is max(100 delta_loop, 1e-13) with delta_loop from the longdouble run on the SAME fp64 box matrices and
the perturbed run: the loop's own rounding, 1e-13 to 2.6e-12.  Measured on the MI355X: tests/README_krylov_scale.md."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from perphil_amd import _ffi  # noqa: E402
import asm_scale_reference as R  # noqa: E402
import krylov_reference as K  # noqa: E402

pytestmark = pytest.mark.gpu

CF = R.CF
KSP = {"cg": _ffi.KSP_CG, "gmres": _ffi.KSP_GMRES}
PC = {"none": _ffi.PC_NONE, "jacobi": _ffi.PC_JACOBI, "block2": _ffi.PC_BLOCK2}


def _cfg(ksp, pc, restart, max_it, rtol=0.0, atol=0.0):
    c = _ffi.SolverCfg()
    c.ksp_type, c.pc_type, c.restart, c.max_it = KSP[ksp], PC[pc], max(restart, 1), max_it
    c.rtol, c.atol = rtol, atol
    c.inner_ksp_type, c.inner_pc_type, c.inner_max_it = _ffi.KSP_CG, _ffi.PC_JACOBI, 100
    c.inner_rtol, c.inner_atol = 1e-12, 1e-300
    c.picard, c.picard_rtol, c.picard_atol, c.picard_max_it = 0, 1e-8, 1e-12, 100
    c.mg_smooth = 2
    return c


_ctx_cache = {}


def _context(make, c, options=()):
    """One assembled context per (mesh, option set) at a time; the mesh's reference stays in krylov_reference's cache."""
    key = (c["kind"], c["nd"], int(c["free"].sum()), tuple(options))
    if _ctx_cache.get("key") != key:
        if "ctx" in _ctx_cache:
            _ctx_cache["ctx"].close()
        _ctx_cache.clear()
        ctx = make()
        for name, v in options:
            ctx.set_option(name, v)
        nd = c["nd"]
        ctx.mesh_build(len(nd), c["kind"], nd[0], nd[1], nd[2] if len(nd) == 3 else 0)
        assert ctx.n == c["n"]
        for f in (0, 1):
            ctx.set_dirichlet(f, c["nodes"][f], c["g"][f][c["nodes"][f]])
        ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True)
        _ctx_cache.update(key=key, ctx=ctx)
    return _ctx_cache["ctx"]


def _close():
    if "ctx" in _ctx_cache:
        _ctx_cache["ctx"].close()
    _ctx_cache.clear()


AGAINST = ("matrix-free", "device-matrix")


def _device_matrix(ctx):
    """The monolithic CSR the context solves with, kept with the context."""
    if "A" not in _ctx_cache:
        _ctx_cache["A"] = ctx.csr(_ffi.MAT_MONO)
    return _ctx_cache["A"]


def _want(c, ctx, loop, against, rtol=0.0, atol=0.0):
    """(the restatement's result to compare with, its bars).  matrix-free: max(100 delta, 1e-13), delta holding the fp64 form of
    the operator against the operator; device-matrix: both sides hold one stored operator, and the bar is that of the loop's own
    rounding alone, max(100 delta_loop, 1e-13) (krylov_reference.reference)."""
    ref = K.reference(c, *loop, rtol, atol)
    assert ref["same_count"]
    if against == "device-matrix":
        return K.run_on_matrix(_device_matrix(ctx), c["b"], *loop, rtol, atol), ref["bars_loop"]
    return ref["out"], ref["bars"]


def _compare(tag, c, ctx, loop, rtol=0.0, atol=0.0, against="matrix-free"):
    """One device run of a loop against the restatement.  Returns (fraction of the history's bar, of the iterate's bar, x, hist);
    the exact properties are asserted here.

    against "matrix-free": the fp64 restatement on the products of asm_scale_reference.System, under ref["bars"].  against
    "device-matrix": the same loop in fp64 on the matrix the context assembled (exported CSR, preconditioner vectors from its
    own diagonals), under ref["bars_loop"], never the wider: what is left is the loop and its vector kernels alone, without the
    difference between two fp64 roundings of the operator (tests/README_krylov_scale.md)."""
    ksp, pc, restart, max_it = loop
    ref = K.reference(c, ksp, pc, restart, max_it, rtol, atol)
    out, (bar_h, bar_x) = _want(c, ctx, loop, against, rtol, atol)
    x, info, hist = ctx.solve_rhs(_cfg(ksp, pc, restart, max_it, rtol, atol), c["b_full"], hist_cap=max_it + 1, raise_on_diverged=False)
    fh, fx = K.hist_distance(hist, out.hist) / bar_h, K.x_distance(x, out.x) / bar_x
    print(f"{tag} {ksp} {pc} restart {restart} max_it {max_it} against {against}: {info.iterations} iterations, hist[-1] {hist[-1]:.6e}; delta hist "
          f"{ref['delta_hist']:.1e} x {ref['delta_x']:.1e} (the loop's rounding alone {ref['delta_loop'][0]:.1e} x {ref['delta_loop'][1]:.1e}); bars {bar_h:.1e} / {bar_x:.1e}; worst fraction: history {fh:.3f}, iterate {fx:.3f}")
    assert info.iterations == out.iterations and len(hist) == out.iterations + 1, (tag, loop, info.iterations, out.iterations)
    assert info.converged == int(out.converged), (tag, loop)
    assert info.resnorm == hist[-1], (tag, loop)
    assert not x[~c["free"]].any()
    return fh, fx, x, hist


# -- the large cases -----------------------------------------------------------------------------------------------------------
LARGE_RUNS = [(m, loop, a) for m in K.LARGE for loop in K.LOOPS[m] for a in AGAINST]


def _side_of_the_caps(mesh, c, loop):
    """Which side of each cap this case is on, from the restated launch rules."""
    n, N = c["n"], 2 * c["n"]
    L, B = K.la_launch(N), K.block2_launch(n)
    ksp, pc, restart, max_it = loop
    if mesh == "quad1024x512":
        assert N == 1051650 and (L["grid"], L["passes"], L["last"]) == (2048, 3, 3074)
        assert (L["red_grid"], L["red_passes"], L["red_last"], L["partials"]) == (1024, 5, 3074, 1024)
        assert (B["build_grid"], B["build_passes"], B["build_last"]) == (2048, 2, 1537) and B["passes"] == 2
        if ksp == "gmres":
            assert (restart, max_it) == (7, 10)
            assert [K.mdot_widths(k + 1) for k in range(7)] == [(1,), (2,), (2, 1), (4,), (4, 1), (4, 2), (4, 2, 1)]
    elif mesh == "quad2048x512":
        assert n == 1051137 and (B["grid"], B["passes"], B["last"]) == (2048, 3, 2561) and L["passes"] == 5 and pc == "block2"
    else:
        assert N == 1090050 and L["passes"] == 3
        Sp = K.spmv_launch(N, 54)
        assert (Sp["lanes"], Sp["grid"], Sp["chunks"], Sp["steps"]) == (8, 1024, 34065, 2) and Sp["passes"] >= 33
    return L, B


@pytest.mark.parametrize("mesh,loop,against", LARGE_RUNS, ids=[f"{m}-{lp[0]}-{lp[1]}-{a}" for m, lp, a in LARGE_RUNS])
def test_krylov_loops_past_the_launch_caps(gpu_ctx_factory, mesh, loop, against):
    """Measured (history / iterate, fractions of the bars; matrix-free | device-matrix):
      quad 1024x512  GMRES none 0.011 / 0.014 | 0.002 / 0.028; jacobi 0.053 / 0.050 | 0.003 / 0.014; block2 0.050 / 0.050 | 0.003 / 0.007
                     CG none 0.011 / 0.011 | 0.001 / 0.003; jacobi 0.056 / 0.055 | 0.004 / 0.007; block2 0.056 / 0.056 | 0.012 / 0.022
      quad 2048x512  CG block2 0.136 / 0.132 | 0.004 / 0.007; GMRES block2 0.004 / 0.051 | 0.000 / 0.004
      hex 128x64x64  CG jacobi 0.007 / 0.007 | 0.002 / 0.003
    Jacobi-CG and block2-CG on quad 1024x512 are 3.5e-13 from the matrix-free restatement (bars 6.2e-12: the fp64 restatement is
    6.2e-14 from its longdouble run) and 4.5e-16 from the same loop on the device's own matrix (bars 1.0e-13)."""
    t0 = time.time()
    kind, nd = K.LARGE[mesh]
    c = K.setup(kind, nd)
    L, B = _side_of_the_caps(mesh, c, loop)
    tail = K.tail_mask(2 * c["n"], L["last"])
    assert np.count_nonzero(c["b"][tail]) > 0      # the last pass holds free rows on which b is nonzero (counts: the host file)
    ctx = _context(gpu_ctx_factory, c)
    t1 = time.time()
    fh, fx, _, _ = _compare(mesh, c, ctx, loop, against=against)
    t2 = time.time()
    print(f"{mesh}: 2n-long kernels {L['grid']} x 256 threads, {L['passes']} passes, last {L['last']} rows; reductions {L['partials']} partial sums, "
          f"{L['red_passes']} passes; k_block2_build {B['build_passes']} passes (last {B['build_last']}), k_block2 {B['passes']} passes (last {B['last']}); "
          f"{t2 - t0:.1f} s, of which mesh + assembly {t1 - t0:.1f} s")
    if (mesh, loop, against) == LARGE_RUNS[-1]:
        _close()
    assert fh <= 1.0 and fx <= 1.0, (mesh, loop, against, fh, fx)


OPTION_SETS = {"fetch_spin0": (("fetch_spin", 0),), "spmv_lanes16": (("spmv_lanes", 16),), "spmv_blocks2048": (("spmv_blocks", 2048),),
               "l3_order_min_rows1000": (("l3_order_min_rows", 1000),)}
OPTION_LOOPS = (("cg", "jacobi", 0, 6), ("gmres", "jacobi", 7, 10))


@pytest.mark.parametrize("against", AGAINST)
@pytest.mark.parametrize("opts", list(OPTION_SETS))
def test_option_sets_on_quad1024x512(gpu_ctx_factory, opts, against):
    """One Jacobi-CG and one Jacobi-GMRES run per option set, under the bars of the default run (the references are shared with
    it).  l3_order_min_rows 1000 puts k_set, k_copy and k_sub of the 2n-long vectors in descending order: history and iterate must
    be the default run's bit for bit (measured: it is, both loops, both references).

    Measured: the Jacobi-GMRES run is at 0.053 / 0.050 of the bars (matrix-free) and 0.003 / 0.014 (device-matrix) under every option
    set; the Jacobi-CG run at 0.002 to 0.007 / 0.005 to 0.013 against the device's matrix and at 0.056 / 0.055 against the
    matrix-free restatement (3.46e-13 to 3.47e-13 of 6.2e-12) under every option set."""
    t0 = time.time()
    mesh = "quad1024x512"
    kind, nd = K.LARGE[mesh]
    c = K.setup(kind, nd)
    N = 2 * c["n"]
    assert K.la_launch(N)["passes"] == 3
    if opts == "spmv_lanes16":
        assert K.spmv_launch(N, 18, lanes=16)["lanes"] == 16 and K.spmv_launch(N, 18)["lanes"] == 8
    if opts == "spmv_blocks2048":
        assert K.spmv_launch(N, 18, blocks=2048)["partials"] == 2048 and K.spmv_launch(N, 18)["partials"] == 1024
    default = {}
    if opts == "l3_order_min_rows1000":
        assert N >= 1000 and N < 4000000        # below the option's default threshold, above this one
        ctx = _context(gpu_ctx_factory, c)
        for loop in OPTION_LOOPS:
            default[loop] = _compare(f"{mesh} default", c, ctx, loop, against=against)[2:]
    ctx = _context(gpu_ctx_factory, c, OPTION_SETS[opts])
    worst = []
    for loop in OPTION_LOOPS:
        fh, fx, x, hist = _compare(f"{mesh} {opts}", c, ctx, loop, against=against)
        worst.append((fh, fx))
        if default:
            assert np.array_equal(hist, default[loop][1]) and np.array_equal(x, default[loop][0]), (opts, loop)
    _close()
    print(f"{mesh} {opts} against {against}: {time.time() - t0:.1f} s")
    assert all(fh <= 1.0 and fx <= 1.0 for fh, fx in worst), worst


# -- the small cases -----------------------------------------------------------------------------------------------------------
SMALL = {"quad1x1": (R.QUAD, (1, 1)), "quad1x2": (R.QUAD, (1, 2)), "hex1x2x1": (R.HEX, (1, 2, 1)), "quad5x3": (R.QUAD, (5, 3)),
         "tet3x4x2": (R.TET, (3, 4, 2)), "quad37x23": (R.QUAD, (37, 23))}
# (restart, max_it): inside a cycle, equal to the restart, restart + 1 (a one-column second cycle)
GMRES_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (30, 3), (30, 30), (30, 31)]
CG_ITS = (1, 2, 5)
NONDEGENERATE = 1e-8      # a loop whose reference history falls below this fraction of hist[0] has nothing left to iterate on
# A cycle of 30 columns exhausts the five small meshes (at most 40 free rows; the preconditioned loops reach 1e-16 hist[0] in about
# 20 steps there, and iterating on divides rounding by rounding): the full cycle of restart 30 and its one-column second cycle
# run on quad 37x23 (1735 free rows), which exists for them.
FULL_CYCLE_MESH = "quad37x23"


def small_loops(mesh: str, free: int):
    """The loops of a small mesh with `free` unconstrained rows.  The Krylov space of a cycle is exhausted at dimension `free`, so
    only loops whose cycles stay below it are run; that what remains has something to iterate on is asserted on the reference."""
    if mesh == FULL_CYCLE_MESH:
        return [("gmres", pc, rs, mi) for pc in ("none", "jacobi", "block2") for rs, mi in GMRES_SHAPES if rs == 30] + [("cg", "jacobi", 0, 5)]
    out = []
    for pc in ("none", "jacobi", "block2"):
        out += [("gmres", pc, rs, mi) for rs, mi in GMRES_SHAPES if min(rs, mi) < min(free, 30)]
        out += [("cg", pc, 0, mi) for mi in CG_ITS if mi < free]
    return out


@pytest.mark.parametrize("against", AGAINST)
@pytest.mark.parametrize("mesh", [m for m in SMALL if m != "quad1x1"])
def test_small_meshes(gpu_ctx_factory, mesh, against):
    t0 = time.time()
    kind, nd = SMALL[mesh]
    c = K.setup(kind, nd)
    free = int(c["free"].sum())
    loops = small_loops(mesh, free)
    assert len(loops) >= 6
    assert K.la_launch(2 * c["n"])["grid"] < K.EW_MAX_WG and K.la_launch(2 * c["n"])["passes"] <= 2       # far below every cap
    ctx = _context(gpu_ctx_factory, c)
    worst = [0.0, 0.0]
    for loop in loops:
        ref = K.reference(c, *loop)
        assert ref["hist"].min() > NONDEGENERATE * ref["hist"][0], (mesh, loop)
        fh, fx, _, _ = _compare(mesh, c, ctx, loop, against=against)
        worst = [max(worst[0], fh), max(worst[1], fx)]
    # max_it = 0: no iteration, x = 0, hist = [beta]; hist_cap below iterations + 1: only hist_cap entries
    for ksp, pc in (("cg", "jacobi"), ("gmres", "jacobi"), ("cg", "block2"), ("gmres", "none")):
        want, bars = _want(c, ctx, (ksp, pc, 2, 0), against)
        x, info, hist = ctx.solve_rhs(_cfg(ksp, pc, 2, 0), c["b_full"], hist_cap=4, raise_on_diverged=False)
        assert info.iterations == 0 and info.converged == 0 and not x.any() and len(hist) == 1 and info.resnorm == hist[0]
        assert want.iterations == 0 and not want.converged and len(want.hist) == 1
        worst[0] = max(worst[0], K.hist_distance(hist, want.hist) / bars[0])
        if free > 2:
            want, bars = _want(c, ctx, (ksp, pc, 2, 2), against)
            x, info, hist = ctx.solve_rhs(_cfg(ksp, pc, 2, 2), c["b_full"], hist_cap=2, raise_on_diverged=False)
            assert info.iterations == 2 and len(hist) == 2
            worst[0] = max(worst[0], K.hist_distance(hist, want.hist[:2]) / bars[0])
            worst[1] = max(worst[1], K.x_distance(x, want.x) / bars[1])
            x, info, hist = ctx.solve_rhs(_cfg(ksp, pc, 2, 2), c["b_full"], hist_cap=0, raise_on_diverged=False)
            assert info.iterations == 2 and len(hist) == 0
    # b = 0: converged at 0 iterations, hist = [0], no NaN in x
    for ksp, pc in (("cg", "jacobi"), ("gmres", "block2")):
        x, info, hist = ctx.solve_rhs(_cfg(ksp, pc, 2, 5), np.zeros(2 * c["n"]), hist_cap=6)
        assert info.iterations == 0 and info.converged == 1 and list(hist) == [0.0] and not x.any() and not np.isnan(x).any()
    _close()
    print(f"{mesh} against {against}: {free} free rows, {len(loops)} loops; worst fraction of the bars: history {worst[0]:.3f}, iterate {worst[1]:.3f}; {time.time() - t0:.1f} s")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


def test_every_node_constrained(gpu_ctx_factory):
    """quad 1x1 with all four nodes in both Dirichlet sets: whatever b holds, F b = 0, and the solve returns x = 0, converged at
    0 iterations, hist = [0], on every loop."""
    kind, nd = SMALL["quad1x1"]
    c = K.setup(kind, nd, constrain_all=True)
    assert not c["free"].any() and not c["b"].any() and c["b_full"].all()
    ctx = _context(gpu_ctx_factory, c)
    for ksp, pc, restart in (("cg", "none", 0), ("cg", "jacobi", 0), ("cg", "block2", 0), ("gmres", "none", 1), ("gmres", "jacobi", 2), ("gmres", "block2", 30)):
        out = K.run(c, ksp, pc, restart, 3)
        assert out.iterations == 0 and out.converged and list(out.hist) == [0.0]
        x, info, hist = ctx.solve_rhs(_cfg(ksp, pc, restart, 3), c["b_full"], hist_cap=4)
        assert info.iterations == 0 and info.converged == 1 and info.resnorm == 0.0 and list(hist) == [0.0]
        assert not x.any() and not np.isnan(x).any()
    _close()


STOP_MESHES = ("quad5x3", "tet3x4x2")
STOP_TOL = 1e-6


@pytest.mark.parametrize("mesh", STOP_MESHES)
def test_stopping_by_tolerance(gpu_ctx_factory, mesh):
    """rtol = 1e-6, and an atol of the same size (1e-6 hist[0] of the reference): the device stops at the restatement's iteration.
    No entry of the reference history lies within 100 bars of the tolerance (asserted), so the two cannot fall on different
    sides of it while the device is within its bar."""
    kind, nd = SMALL[mesh]
    c = K.setup(kind, nd)
    ctx = _context(gpu_ctx_factory, c)
    # (CG without a preconditioner needs as many iterations as there are free rows to get there: no stopping test in that)
    for ksp, pc, restart in (("cg", "jacobi", 0), ("cg", "block2", 0), ("gmres", "none", 30), ("gmres", "jacobi", 30),
                             ("gmres", "block2", 30), ("gmres", "jacobi", 2)):
        free_run = K.reference(c, ksp, pc, restart, 200, STOP_TOL, 0.0)
        beta = float(free_run["hist"][0])
        for rtol, atol in ((STOP_TOL, 0.0), (0.0, STOP_TOL * beta)):
            ref = K.reference(c, ksp, pc, restart, 200, rtol, atol)
            out = ref["out"]
            tol = max(rtol * beta, atol)
            assert out.converged and 0 < out.iterations < 200 and ref["same_count"]
            assert (abs(ref["hist"] - tol) > 100.0 * ref["bars"][0] * ref["hist"]).all(), (mesh, ksp, pc, restart)
            x, info, hist = ctx.solve_rhs(_cfg(ksp, pc, restart, 200, rtol, atol), c["b_full"], hist_cap=201)
            print(f"{mesh} {ksp} {pc} restart {restart} rtol {rtol:g} atol {atol:.3g}: {info.iterations} iterations (reference {out.iterations}), "
                  f"history {K.hist_distance(hist, ref['hist']) / ref['bars'][0]:.3f} of its bar, iterate {K.x_distance(x, ref['x']) / ref['bars'][1]:.3f}")
            assert info.iterations == out.iterations and info.converged == 1 and info.resnorm == hist[-1] and hist[-1] <= tol
    _close()
