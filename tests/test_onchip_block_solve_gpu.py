"""The on-chip LU-equivalent block solves (`k_coarse_cg_sell` through `mg_onchip_cg`: every block solve of the
direct-equivalent configurations on blocks of at most 4096 rows) against their NumPy restatement (`onchip_cg_reference.py`,
checked on the host by `test_onchip_block_solve_host.py`) and the sparse direct solution, on every branch of the kernel:
both launch sizes, 4 rows per thread, the threshold from both sides, ragged boxes, all four stencils, full and symmetric
storage, all-constrained blocks, high contrast - and the report of a solve that stops short (pph_solve_info.inner_failed).

Every solve goes through `ctx.solve` with what `translate_options` makes of LINEAR_SOLVER_PARAMS ("direct") and of
{**GMRES_PARAMS, **FIELDSPLIT_LU_PARAMS} ("fieldsplit_lu"), manufactured Dirichlet data on the whole boundary.  The system is
assembled WITH the monolithic matrix, as `solve_dpp` assembles it for these option sets: the outer GMRES runs on it, and
pph_solve refuses a Krylov solve without it.

Each case prints what it measured next to its bound; the figures are copied into the table of tests/README.md."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import onchip_cg_reference as R  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [R.case_id(lbl, c) for lbl, c in R.CASES]


def _cfg(preset):
    from perphil_amd import solver_parameters as spar
    from perphil_amd.solver import translate_options

    params = spar.LINEAR_SOLVER_PARAMS if preset == "direct" else {**spar.GMRES_PARAMS, **spar.FIELDSPLIT_LU_PARAMS}
    return translate_options(params)[0]


def _ctx(make, label, coeffs, **options):
    _, dim, kind, nx, ny, nz = R._BY_LABEL[label]
    om, _ = R.system(label, coeffs)
    p = R.params_of(coeffs)
    ctx = make()
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.mesh_build(dim, kind, nx, ny, nz)
    b = o.boundary_nodes(om)
    e1, e2 = o.exact_pressures(om.coords, p)
    ctx.set_dirichlet(0, b, e1[b])
    ctx.set_dirichlet(1, b, e2[b])
    ctx.assemble(p.k1, p.k2, p.beta, p.mu, monolithic=True)
    return ctx


def _check_solution(tag, x, label, coeffs, preset):
    err, bound = R.rel_max_error(x, R.direct_solution(label, coeffs)), R.solution_bound(label, coeffs, preset)
    print(f"{tag}: max |x - u_direct| / max |u_direct| = {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    return err


def _check_history(hist, label, coeffs, preset):
    """Outer preconditioned residual norms against the same GMRES with sparse-LU block solves, to the rtol 1e-5 of
    test_G9_fieldsplit_gmres, over the entries above 1e-9 of entry 0 (below, the 1e-12 of the block solves shows)."""
    ref = np.array(R.exact_block_history(label, coeffs, preset))
    m = min(int((ref > 1e-9 * ref[0]).sum()), len(hist), len(ref))
    assert m == int((ref > 1e-9 * ref[0]).sum()) or m == len(hist)
    np.testing.assert_allclose(hist[:m], ref[:m], rtol=1e-5)
    return m


def _check_counts(tag, info, t, label, coeffs, preset):
    """Outer count: the restatement's exactly, except where the restatement itself says the crossing of the tolerance is
    decided by rounding (onchip_cg_reference.outer_counts_allowed: the block solves are accurate to 1e-12 of the first
    residual only, so a residual norm within that distance of the tolerance - always the case for the direct preset, whose
    tolerance 1e-13 lies below it - can cross one iteration earlier or later under another summation order).  Block CG
    iterations: summed, within +-2 per block solve of the restatement's over the same block solves."""
    rs = R.restated_solve(label, coeffs, preset)
    its, solves, cg = int(info.iterations), t["onchip_solves"], t["onchip_cg_iterations"]
    print(f"{tag}: outer {its} (restated {rs.outer_its}, allowed {rs.outer_its_allowed}), on-chip solves {solves}, "
          f"unconverged {t['onchip_unconverged']}, CG iterations {cg} (restated {rs.stats.cg_iterations})")
    assert its in rs.outer_its_allowed
    assert solves == 2 * (its + 1)              # P^-1 b, then one application per outer iteration (no restart below 30)
    assert its < 30
    ref = rs.stats.per_solve
    common = min(solves, len(ref))
    lo, hi = sum(ref[:common]) - 2 * common, sum(ref[:common]) + 2 * common
    if solves > len(ref):                        # one more application than the restatement ran: its two solves on top
        hi += 2 * (max(ref) + 2)
    assert lo <= cg <= hi


@pytest.mark.parametrize("label,coeffs", R.CASES, ids=IDS)
def test_onchip_solves_match_restatement(gpu_ctx_factory, label, coeffs):
    onchip = R.NODES[label] <= R.ONCHIP_MAX_ROWS
    ctx = _ctx(gpu_ctx_factory, label, coeffs)
    assert ctx.n == R.NODES[label]
    for preset in R.PRESETS:
        tag = f"{R.case_id(label, coeffs)} {preset}"
        x, info, hist = ctx.solve(_cfg(preset), hist_cap=64)
        t = ctx.timers()
        assert info.converged and not info.inner_failed
        if onchip:
            assert t["onchip_solves"] > 0 and t["onchip_unconverged"] == 0
            _check_counts(tag, info, t, label, coeffs, preset)
        else:
            # just past the threshold: the host-driven multigrid-CG, whose iterations are counted one by one
            assert (t["onchip_solves"], t["onchip_unconverged"], t["onchip_cg_iterations"]) == (0, 0, 0)
            assert info.iterations in R.restated_solve(label, coeffs, preset).outer_its_allowed
            assert info.inner_iterations > 2 * (info.iterations + 1)
        _check_solution(tag, x, label, coeffs, preset)
        m = _check_history(hist, label, coeffs, preset)
        print(f"{tag}: {m} residual norms equal to the exact-block GMRES's to 1e-5")


@pytest.mark.parametrize("label", ["quad 63x63", "hex 5x4x6"])
def test_csr_blocks_do_not_run_on_chip(gpu_ctx_factory, label):
    """op_format 0: no stencil-ELL values, so the block solves are the host-driven multigrid-CG; same bound."""
    ctx = _ctx(gpu_ctx_factory, label, R.BASE_COEFFS, op_format=0)
    for preset in R.PRESETS:
        x, info, hist = ctx.solve(_cfg(preset), hist_cap=64)
        t = ctx.timers()
        assert info.converged and not info.inner_failed
        assert (t["onchip_solves"], t["onchip_unconverged"], t["onchip_cg_iterations"]) == (0, 0, 0)
        _check_solution(f"{label} op_format 0 {preset}", x, label, R.BASE_COEFFS, preset)
        _check_history(hist, label, R.BASE_COEFFS, preset)


@pytest.mark.parametrize("label", ["hex 15x15x15", "quad 63x63", "tet 7x9x5"])
def test_full_and_symmetric_storage_agree(gpu_ctx_factory, label):
    """sell_sym 1 reads the lower entries from the mirror slot of the neighbouring row: same entries, same order of the
    row sum, so the two storages meet the same bound and agree to 1e-12 of max |u|."""
    ud = R.direct_solution(label, R.BASE_COEFFS)
    xs = {}
    for sym in (0, 1):
        ctx = _ctx(gpu_ctx_factory, label, R.BASE_COEFFS, sell_sym=sym)
        for preset in R.PRESETS:
            x, info, _ = ctx.solve(_cfg(preset))
            t = ctx.timers()
            assert t["symmetric_storage"] == bool(sym)
            assert info.converged and t["onchip_solves"] > 0 and t["onchip_unconverged"] == 0
            _check_solution(f"{label} sell_sym {sym} {preset}", x, label, R.BASE_COEFFS, preset)
            xs[(sym, preset)] = x.copy()
    for preset in R.PRESETS:
        d = np.abs(xs[(0, preset)] - xs[(1, preset)]).max() / np.abs(ud).max()
        print(f"{label} {preset}: full against symmetric storage {d:.2e}")
        assert d <= 1e-12


def test_threshold_from_both_sides(gpu_ctx_factory):
    """quad 63x63 (4096 rows: on chip, 4 rows per thread) and quad 64x64 (4225: host-driven multigrid-CG) each meet their
    own bound."""
    for label, onchip in (("quad 63x63", True), ("quad 64x64", False)):
        ctx = _ctx(gpu_ctx_factory, label, R.BASE_COEFFS)
        x, info, _ = ctx.solve(_cfg("direct"))
        t = ctx.timers()
        assert info.converged and not info.inner_failed
        assert (t["onchip_solves"] > 0) == onchip
        assert (info.inner_iterations == t["onchip_solves"]) == onchip      # host-driven CG iterations are counted one by one
        _check_solution(f"{label} direct", x, label, R.BASE_COEFFS, "direct")


def test_unconverged_onchip_solve_is_reported(gpu_ctx_factory):
    """onchip_max_it 3: every block solve of hex 15^3 stops at its limit.  The solve says so (inner_failed, the count in
    the timers) instead of reporting iteration_number 1 / residual 0.0 in silence; with the option back at 0 the flag is
    clear and the solution meets its bound again.  Stopping an iteration early faults nothing."""
    label, coeffs = "hex 15x15x15", R.BASE_COEFFS
    ctx = _ctx(gpu_ctx_factory, label, coeffs)
    cfg = _cfg("direct")
    ctx.set_option("onchip_max_it", 3)
    _, info, _ = ctx.solve(cfg, raise_on_diverged=False)
    t = ctx.timers()
    assert info.inner_failed == 1 and not info.converged
    assert t["onchip_solves"] > 0 and t["onchip_unconverged"] == t["onchip_solves"]
    assert t["onchip_cg_iterations"] == 3 * t["onchip_solves"]
    ctx.set_option("onchip_max_it", 0)
    x, info, _ = ctx.solve(cfg, raise_on_diverged=False)
    t = ctx.timers()
    assert info.converged and not info.inner_failed and t["onchip_unconverged"] == 0 and t["onchip_solves"] > 0
    _check_solution(f"{label} direct, onchip_max_it back at 0", x, label, coeffs, "direct")


def _public_problem(kind):
    import perphil_amd as pa
    from perphil_amd import fd

    params = pa.DPPParameters(k1=1.0, k2=1.0 / 1e2, beta=1.0, mu=1.0)
    if kind == "hex":
        mesh = fd.UnitCubeMesh(15, 15, 15, hexahedral=True)
        _, p1e, _, p2e = pa.exact_expressions_3d(mesh, params)
    else:
        mesh = pa.create_mesh(63, 63, quadrilateral=False)
        _, p1e, _, p2e = pa.exact_expressions(mesh, params)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    bcs = [fd.DirichletBC(W.sub(0), p1e, "on_boundary"), fd.DirichletBC(W.sub(1), p2e, "on_boundary")]
    return mesh, W, params, bcs


def _block_solve_warnings(rec):
    # (the once-per-process announcement of the direct-equivalent substitution is not the warning in question)
    return [w for w in rec if "stopped at its iteration limit" in str(w.message)]


@pytest.mark.parametrize("kind,label", [("hex", "hex 15x15x15"), ("tri", "tri 63x63")])
def test_public_api_direct_equivalent_on_chip(gpu_ctx_factory, kind, label):
    import perphil_amd as pa
    from perphil_amd import solver_parameters as spar

    mesh, W, params, bcs = _public_problem(kind)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        sol = pa.solve_dpp(W, params, bcs, solver_parameters=spar.LINEAR_SOLVER_PARAMS)
    assert not _block_solve_warnings(rec)
    assert sol.iteration_number == 1 and sol.residual_error == 0.0 and not sol.info["inner_failed"]
    assert sol.info["timers"]["onchip_solves"] > 0 and sol.info["timers"]["onchip_unconverged"] == 0
    _check_solution(f"solve_dpp {label} LINEAR_SOLVER_PARAMS", sol.solution.vector(), label, R.BASE_COEFFS, "direct")


def test_public_api_warns_about_unconverged_onchip_solves(gpu_ctx_factory):
    """solve_dpp with LINEAR_SOLVER_PARAMS and onchip_max_it 3 on hex 15^3: the warning of a truncated coarsest multigrid
    solve, whether the outer iteration still converges (then next to iteration_number 1 / residual 0.0) or not (then before
    the ConvergenceError)."""
    import perphil_amd as pa
    from perphil_amd import _ffi, solver_parameters as spar

    mesh, W, params, bcs = _public_problem("hex")
    mesh.context().set_option("onchip_max_it", 3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        try:
            sol = pa.solve_dpp(W, params, bcs, solver_parameters=spar.LINEAR_SOLVER_PARAMS)
            assert sol.info["inner_failed"]
        except _ffi.ConvergenceError:
            pass
    assert _block_solve_warnings(rec)
    mesh.context().set_option("onchip_max_it", 0)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        sol = pa.solve_dpp(W, params, bcs, solver_parameters=spar.LINEAR_SOLVER_PARAMS)
    assert not _block_solve_warnings(rec) and not sol.info["inner_failed"]
    _check_solution("solve_dpp hex 15x15x15, onchip_max_it back at 0", sol.solution.vector(), "hex 15x15x15", R.BASE_COEFFS, "direct")
