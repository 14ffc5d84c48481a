"""The CG-1 multigrid V-cycle itself, per application, on every branch of perphil_amd/csrc/pph_mg.hip.

Part 1: z = pph_pc_apply(mg) on a degree-1 context against oracle.dpp_mg_oracle (tests/mg_cycle_reference.py) for a random
vector and for vectors on which one level dominates (r = A_0 P_0 ... P_{l-1} e), mg_smooth 1 (fused cycle: k_restrict_q1 /
k_restrict with the coarse pre-smoothing, k_prolong_to_q1 / k_prolong_to, k_mg_tail) and 2 (general cycle), both blocks,
max |z - ref| <= 1e-10 max |ref|, z = 0 on constrained entries, a second call bit-identical, fused against general cycle to
1e-12.  Every case asserts the branch it reaches from the launch rules restated in mg_cycle_reference (level sizes ->
mg_tail_begin / mg_tail_lds, work items -> mg_grid) and prints mesh, level sizes, first tail level, NL, branch, worst
error and bound.

Part 2: the cycle as the Krylov loop calls it (pre-smoothed first guess, r.z from the last Jacobi-epilogue product): one
Picard sweep of exactly k = 1, 2, 3 PCG iterations per block (inner_norm 2), far from converged, against the same
iterations in NumPy.

tests/test_mg_cycle_host.py shows that these comparisons reject cycles that are wrong by a little."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mg_cycle_reference as MC  # noqa: E402
from oracle import dpp_mg_oracle as G  # noqa: E402

from perphil_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu

K1, K2, BETA, MU = MC.K1, MC.K2, MC.BETA, MC.MU
_levels_cache = {}


def _levels(kind, nx, ny, nz, which, variant, coefs=(K1, K2, BETA), matfree=False):
    key = (kind, nx, ny, nz, which, variant, coefs, matfree)
    if key not in _levels_cache:
        n = MC.level_nodes(kind, nx, ny, nz)[0]
        mask = MC.mask_of(n, MC.dirichlet_nodes(kind, nx, ny, nz, variant, which))
        cK, cM = coefs[which] / MU, coefs[2] / MU
        if matfree:
            lv = MC.matfree_hierarchy(kind, nx, ny, nz, cK, cM, mask)
        else:
            lv = G.build_hierarchy(MC.dim_of(kind), kind, nx, ny, nz, cK, cM, mask)
        _levels_cache[key] = lv
    return _levels_cache[key]


def _set_data(ctx, kind, nx, ny, nz, variant, coefs=(K1, K2, BETA)):
    for f in (0, 1):
        nodes = MC.dirichlet_nodes(kind, nx, ny, nz, variant, f)
        ctx.set_dirichlet(f, nodes, MC.dirichlet_values(kind, nx, ny, nz, nodes, f))
    ctx.assemble(coefs[0], coefs[1], coefs[2], MU, monolithic=False)


def _new_ctx(make, kind, nx, ny, nz, variant=0, options=()):
    ctx = make()
    for name, value in options:
        ctx.set_option(name, value)
    ctx.mesh_build(MC.dim_of(kind), kind, nx, ny, nz)
    _set_data(ctx, kind, nx, ny, nz, variant)
    return ctx


def _branch(kind, nx, ny, nz, expect, tail_rows=MC.MG_TAIL_ROWS_DEFAULT, coarse_on_device=True):
    """The branch of the fused cycle on this mesh from the restated launch rules; `expect` must be part of it."""
    b = MC.branch_of(kind, nx, ny, nz, tail_rows, coarse_on_device)
    for key, want in expect.items():
        assert b[key] == want, (key, b)
    return b


def _check(ctx, kind, nx, ny, nz, variant, branch, label, coefs=(K1, K2, BETA), matfree=False, smooths=(1, 2), blocks=(0, 1),
           probes=True, seed=11, general_too=True, bound=MC.CYCLE_BOUND):
    """One application per probing vector, block and mg_smooth against the reference; returns {(which, ns): worst error}."""
    assert ctx.n == branch["levels"][0]
    out = {}
    for which in blocks:
        lv = _levels(kind, nx, ny, nz, which, variant, coefs, matfree)
        assert [l.mask.size for l in lv] == branch["levels"]
        mask = lv[0].mask
        vectors = MC.probe_vectors(lv, seed + which)
        if not probes:
            vectors = vectors[:1]
        for ns in smooths:
            worst = (0.0, "")
            for name, r in vectors:
                ref = MC.apply_reference(lv, r, ns)
                rd = r.copy()
                rd[mask] = 7.0                                     # the entry point clears constrained entries itself
                z = ctx.pc_apply(which, _ffi.PC_MG, rd, mg_smooth=ns)
                err = MC.rel_err(z, ref)
                worst = max(worst, (err, name))
                assert err <= bound, (label, which, ns, name, err)
                assert not z[mask].any()
                if name.startswith("random"):
                    assert np.array_equal(z, ctx.pc_apply(which, _ffi.PC_MG, rd, mg_smooth=ns))
                if ns == 1 and general_too and len(lv) > 1:
                    ctx.set_option("mg_fused", 0)
                    zg = ctx.pc_apply(which, _ffi.PC_MG, rd, mg_smooth=1)
                    ctx.set_option("mg_fused", 1)
                    eg, ef = MC.rel_err(zg, ref), MC.rel_err(z, zg)
                    assert eg <= bound, (label, which, "general cycle", name, eg)
                    assert ef <= MC.FUSED_BOUND, (label, which, "fused against general cycle", name, ef)
            out[(which, ns)] = worst[0]
            print(f"{label}: {MC.KIND_NAME[kind]} {nx}x{ny}x{nz} levels {branch['levels']} first tail level {branch['lt']} NL {branch['NL']} "
                  f"coarsest: {branch['coarsest']}; block {which} mg_smooth {ns}: worst |z - ref| / |ref| = {worst[0]:.2e} ({worst[1]}), "
                  f"bound {bound:.0e}")
    return out


# mesh -> what the restated rules must say about it
CASES = {
    "quad64": (MC.QUAD, 64, 64, 0, {"NL": 4, "lt": 2, "coarsest": "tail, one-wave CG"}),
    "tri64": (MC.TRI, 64, 64, 0, {"NL": 4, "lt": 2, "coarsest": "tail, one-wave CG"}),
    "quad40x36": (MC.QUAD, 40, 36, 0, {"NL": 2, "lt": 1, "coarsest": "tail, workgroup CG"}),
    "tri40x36": (MC.TRI, 40, 36, 0, {"NL": 2, "lt": 1, "coarsest": "tail, workgroup CG"}),
    "hex16": (MC.HEX, 16, 16, 16, {"NL": 3, "lt": 1, "coarsest": "tail, one-wave CG"}),
    "tet16": (MC.TET, 16, 16, 16, {"NL": 3, "lt": 1, "coarsest": "tail, one-wave CG"}),
    "hex20": (MC.HEX, 20, 20, 20, {"NL": 1, "lt": 2, "levels": [9261, 1331, 216], "coarsest": "tail, workgroup CG"}),
    "tet20": (MC.TET, 20, 20, 20, {"NL": 1, "lt": 2, "coarsest": "tail, workgroup CG"}),
    "hex12x8x16": (MC.HEX, 12, 8, 16, {"NL": 2, "lt": 1, "levels": [1989, 315, 60], "coarsest": "tail, one-wave CG"}),
    "tet12x8x16": (MC.TET, 12, 8, 16, {"NL": 2, "lt": 1, "coarsest": "tail, one-wave CG"}),
    "hex32": (MC.HEX, 32, 32, 32, {"NL": 3, "lt": 2, "coarsest": "tail, one-wave CG"}),
    "tet24": (MC.TET, 24, 24, 24, {"NL": 2, "lt": 2, "levels": [15625, 2197, 343, 64], "coarsest": "tail, one-wave CG"}),
    # no coarsening at all: max(steps, 2) Chebyshev steps
    "quad5x3": (MC.QUAD, 5, 3, 0, {"nlev": 1, "coarsest": "chebyshev only"}),
    "tri5x3": (MC.TRI, 5, 3, 0, {"nlev": 1, "coarsest": "chebyshev only"}),
    "hex3x4x2": (MC.HEX, 3, 4, 2, {"nlev": 1, "coarsest": "chebyshev only"}),
    "tet3x4x2": (MC.TET, 3, 4, 2, {"nlev": 1, "coarsest": "chebyshev only"}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_application_against_the_oracle(gpu_ctx_factory, name):
    """Every kind, every tail depth it can reach, the one-wave and the workgroup coarsest CG, level 0 of the tail as the
    coarsest level (NL 1), ragged boxes (odd pxf: the last pair of k_prolong_to_q1 has one node), meshes without coarsening.
    Dirichlet data on part of the boundary plus constrained nodes inside the domain: k_restrict_q1 takes its fast path and
    its masked path in every launch."""
    kind, nx, ny, nz, expect = CASES[name]
    b = _branch(kind, nx, ny, nz, expect)
    if b["nlev"] > 1:
        assert all(px % 2 == 1 for px, _, _ in MC.level_dims(kind, nx, ny, nz)[:-1])      # odd pxf on every fine level
        mask = MC.mask_of(b["levels"][0], MC.dirichlet_nodes(kind, nx, ny, nz, 0, 0))
        i, j, k = MC.node_ijk(kind, nx, ny, nz)
        inside = mask & (i > 0) & (i < nx) & (j > 0) & (j < ny) & ((k > 0) & (k < nz) if MC.dim_of(kind) == 3 else True)
        assert inside.any() and not mask[i == nx].all()
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    _check(ctx, kind, nx, ny, nz, 0, b, name)
    ctx.close()


@pytest.mark.parametrize("name", ["quad64", "tri64", "hex16", "tet16"])
def test_tail_moved_by_options_on_one_context(gpu_ctx_factory, name):
    """Option mg_tail_rows at every value that changes mg_tail_begin (NL from the deepest tail down to 1, then no tail:
    k_coarse_cg_sell), then coarse_on_device 0 (host-driven pph_cg_jacobi), on ONE context: the tail pack follows."""
    kind, nx, ny, nz, expect = CASES[name]
    ns = MC.level_nodes(kind, nx, ny, nz)
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    seen = []
    for rows in sorted(set(ns[1:]), reverse=True) + [0]:
        b = _branch(kind, nx, ny, nz, {}, tail_rows=rows)
        if seen and b["NL"] == seen[-1]:
            continue
        seen.append(b["NL"])
        if b["NL"] == 0:
            assert b["coarsest"] == "k_coarse_cg_sell"
        ctx.set_option("mg_tail_rows", rows)
        _check(ctx, kind, nx, ny, nz, 0, b, f"{name} mg_tail_rows {rows}", smooths=(1,), general_too=False)
    assert seen == list(range(expect["NL"], -1, -1)), seen
    ctx.set_option("mg_tail_rows", MC.MG_TAIL_ROWS_DEFAULT)
    ctx.set_option("coarse_on_device", 0)
    b = _branch(kind, nx, ny, nz, {"NL": 0, "coarsest": "pph_cg_jacobi"}, coarse_on_device=False)
    _check(ctx, kind, nx, ny, nz, 0, b, f"{name} coarse_on_device 0")
    ctx.set_option("coarse_on_device", 1)
    _check(ctx, kind, nx, ny, nz, 0, _branch(kind, nx, ny, nz, expect), f"{name} back to the defaults", smooths=(1,), general_too=False)
    ctx.close()


@pytest.mark.parametrize("name", ["hex16", "quad64", "tet16", "tri40x36"])
def test_hierarchy_follows_dirichlet_sets_and_coefficients(gpu_ctx_factory, name):
    """ONE context: cycle; another Dirichlet set (whole boundary, nothing inside) and re-assembly; other k1, k2, beta - each
    against a freshly built oracle hierarchy: restriction flags, injected masks and the tail pack must not be stale."""
    kind, nx, ny, nz, expect = CASES[name]
    b = _branch(kind, nx, ny, nz, expect)
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz, variant=0)
    _check(ctx, kind, nx, ny, nz, 0, b, f"{name} first set", seed=5)
    _set_data(ctx, kind, nx, ny, nz, 1)
    _check(ctx, kind, nx, ny, nz, 1, b, f"{name} whole boundary", seed=6)
    coefs = (0.3, 2.0, 0.5)
    _set_data(ctx, kind, nx, ny, nz, 1, coefs)
    _check(ctx, kind, nx, ny, nz, 1, b, f"{name} other coefficients", coefs=coefs, seed=7)
    _set_data(ctx, kind, nx, ny, nz, 0, coefs)
    _check(ctx, kind, nx, ny, nz, 0, b, f"{name} first set again", coefs=coefs, seed=8)
    ctx.close()


@pytest.mark.parametrize("name", ["hex12x8x16", "tri40x36", "quad64", "tet16"])
def test_csr_levels_and_fp32_smoother(gpu_ctx_factory, name):
    """op_format 0 (CSR level operators: the general cycle, k_coarse_cg): the same bound.  mg_fp32 1 is fp32 inside the
    smoother: its result is NOT the fp64 one bit for bit and lies within 100 x the discrepancy of the NumPy cycle whose
    smoother and residual products read level operators rounded to fp32 (measured on the host, tests/README.md)."""
    kind, nx, ny, nz, expect = CASES[name]
    b = _branch(kind, nx, ny, nz, expect)
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz, options=[("op_format", 0)])
    _check(ctx, kind, nx, ny, nz, 0, b, f"{name} op_format 0", general_too=False)
    for which in (0, 1):
        lv = _levels(kind, nx, ny, nz, which, 0)
        A32 = MC.fp32_operators(lv)
        for ns in (1, 2):
            for vname, r in MC.probe_vectors(lv, 13):
                ref = MC.apply_reference(lv, r, ns)
                delta = MC.rel_err(MC.apply_reference(lv, r, ns, smooth_A=A32), ref)
                ctx.set_option("mg_fp32", 0)
                z64 = ctx.pc_apply(which, _ffi.PC_MG, r, mg_smooth=ns)
                ctx.set_option("mg_fp32", 1)
                z32 = ctx.pc_apply(which, _ffi.PC_MG, r, mg_smooth=ns)
                err = MC.rel_err(z32, ref)
                print(f"{name} mg_fp32 block {which} mg_smooth {ns} {vname}: |z32 - ref| / |ref| = {err:.2e}, NumPy fp32 operators "
                      f"against fp64 {delta:.2e} (bound 100 x), fp64 device {MC.rel_err(z64, ref):.2e}")
                assert not np.array_equal(z32, z64)
                assert err <= 100 * delta
                assert MC.rel_err(z64, ref) <= MC.CYCLE_BOUND
    ctx.close()


def test_row_dictionaries_inside_the_cycle(gpu_ctx_factory):
    """The products of the cycle on row dictionaries (fine level: walk kernels; coarse levels: their own dictionaries) are
    the stored-value products bit for bit, and one of them is the oracle's cycle."""
    kind, nx, ny, nz, expect = CASES["hex32"]
    b = _branch(kind, nx, ny, nz, expect)
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz, variant=1,
                   options=[("sell_zwalk_min_chunks", 1), ("sell_dict", 1), ("sell_dict_min_rows", 1)])
    t = ctx.timers()
    assert t["dict_operators"] >= 3 and t["dict_status"] == 1, t
    _check(ctx, kind, nx, ny, nz, 1, b, "hex32 on row dictionaries")
    rng = np.random.default_rng(3)
    r = rng.standard_normal(ctx.n)
    with_dict = {(w, ns): ctx.pc_apply(w, _ffi.PC_MG, r, mg_smooth=ns).copy() for w in (0, 1) for ns in (1, 2)}
    assert ctx.timers()["dict_operators"] >= 3
    ctx.set_option("sell_dict", 0)
    _set_data(ctx, kind, nx, ny, nz, 1)
    assert ctx.timers()["dict_operators"] == 0
    for (w, ns), z in with_dict.items():
        assert np.array_equal(z, ctx.pc_apply(w, _ffi.PC_MG, r, mg_smooth=ns)), (w, ns)
    ctx.close()


LARGE = {
    # more than 524 288 pairs in k_prolong_to_q1 on level 0, NL = 4 in 2D at full size
    "quad1024": (MC.QUAD, 1024, 1024, 0, {"NL": 4, "coarsest": "tail, one-wave CG"}),
    # more than 524 288 nodes on level 1: the restriction to it, the interpolation from it and its own sweeps loop
    "hex160": (MC.HEX, 160, 160, 160, {"NL": 1, "levels": [4173281, 531441, 68921, 9261, 1331, 216], "coarsest": "tail, workgroup CG"}),
}


@pytest.mark.parametrize("name", list(LARGE))
def test_grid_stride_loops_against_the_matrix_free_reference(gpu_ctx_factory, name):
    kind, nx, ny, nz, expect = LARGE[name]
    b = _branch(kind, nx, ny, nz, expect)
    dims = MC.level_dims(kind, nx, ny, nz)
    assert MC.loops(MC.q1_pairs(dims[0])) and b["levels"][0] > 1048576
    assert MC.mg_grid(MC.q1_pairs(dims[0])) == MC.MG_GRID_BLOCKS
    if name == "hex160":
        assert MC.loops(b["levels"][1]) and MC.loops(MC.q1_pairs(dims[1])) is False and MC.mg_grid(b["levels"][1]) == MC.MG_GRID_BLOCKS
    t0 = time.time()
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    _check(ctx, kind, nx, ny, nz, 0, b, name, matfree=True, probes=False)
    _check(ctx, kind, nx, ny, nz, 0, b, f"{name} level probes", matfree=True, smooths=(1,), blocks=(1,), seed=19)
    ctx.close()
    _levels_cache.clear()
    print(f"{name}: {time.time() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------------------------------
# part 2: the cycle inside the Krylov loop
# ---------------------------------------------------------------------------------------------------------------------
def _sweep_cfg(k):
    c = _ffi.SolverCfg()
    c.ksp_type, c.pc_type, c.restart, c.max_it = _ffi.KSP_GMRES, _ffi.PC_NONE, 30, 50000
    c.rtol, c.atol = 1e-8, 1e-12
    c.inner_ksp_type, c.inner_pc_type, c.inner_max_it = _ffi.KSP_CG, _ffi.PC_MG, k
    c.inner_rtol, c.inner_atol = 1e-12, 1e-300
    c.picard, c.picard_rtol, c.picard_atol, c.picard_max_it = 1, 1e-8, 1e-12, 1
    c.mg_smooth = 1
    c.inner_norm = 2
    return c


# per kind one mesh whose levels 1.. are all in the tail and one with full-chip levels above the tail
SWEEPS = ["quad40x36", "quad64", "tri40x36", "tri64", "hex16", "hex32", "tet16", "tet24"]


@pytest.mark.parametrize("name", SWEEPS)
def test_unconverged_picard_sweep_against_numpy_pcg(gpu_ctx_factory, name):
    """picard_max_it 1, inner_norm 2, inner_max_it k: exactly k PCG iterations per block with the fused cycle called as the
    loop calls it.  u0 + du after that sweep against k iterations of PCG in NumPy with the oracle's cycle; use_graphs 1
    and 2, fold_finals 0 and 1 (bit-identical to each other).  Bound: 1e-10 max |du| for k = 1; k = 2, 3: 100 x the drift of
    the reference under a permuted numbering (at least 1e-13), computed here on the host."""
    kind, nx, ny, nz, expect = CASES[name]
    b = _branch(kind, nx, ny, nz, expect)
    p = MC.sweep_problem(kind, nx, ny, nz)
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    for k in (1, 2, 3):
        du = MC.sweep_reference(p, k)
        bound = MC.sweep_bound(p, k)
        for graphs in (1, 2):
            ctx.set_option("use_graphs", graphs)
            got = {}
            for fold in (0, 1):
                ctx.set_option("fold_finals", fold)
                x, info, _ = ctx.solve(_sweep_cfg(k), raise_on_diverged=False)
                got[fold] = np.array(x, copy=True)
                assert info.iterations == 1 and info.inner_iterations == 2 * k, (info.iterations, info.inner_iterations)
                err = float(abs(got[fold] - (p["u0"] + du)).max() / abs(du).max())
                print(f"{name} levels {b['levels']} first tail level {b['lt']} NL {b['NL']}: k {k} use_graphs {graphs} fold_finals {fold}: "
                      f"|u - (u0 + du_ref)| / |du_ref| = {err:.2e}, bound {bound:.2e}")
                assert err <= bound, (name, k, graphs, fold, err, bound)
                for f in (0, 1):
                    assert np.array_equal(got[fold][f * p["n"] + p["nodes"][f]], p["values"][f])
            assert np.array_equal(got[0], got[1])
    ctx.close()
