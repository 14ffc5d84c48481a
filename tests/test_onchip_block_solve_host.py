"""The references of `test_onchip_block_solve_gpu.py` (`onchip_cg_reference.py`), checked on the host: the restated on-chip
block solve against a sparse direct solve of the same block, the direct reference solution against its own residual, and the
figures of the restated direct-equivalent solves that the GPU tests take their bounds from (table in tests/README.md)."""
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import onchip_cg_reference as R  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

IDS = [R.case_id(lbl, c) for lbl, c in R.CASES]


def test_presets_are_what_translate_options_produces():
    from perphil_amd import _ffi, solver_parameters as spar
    from perphil_amd.solver import translate_options

    for name, params in (("direct", spar.LINEAR_SOLVER_PARAMS), ("fieldsplit_lu", {**spar.GMRES_PARAMS, **spar.FIELDSPLIT_LU_PARAMS})):
        cfg, _ = translate_options(params)
        kw = R.PRESETS[name]
        assert (cfg.ksp_type, cfg.pc_type, cfg.picard) == (_ffi.KSP_GMRES, _ffi.PC_FIELDSPLIT, 0)
        assert (cfg.rtol, cfg.atol, cfg.max_it, cfg.restart) == (kw["rtol"], kw["atol"], kw["max_it"], kw["restart"])
        assert cfg.inner_exact == 1 and min(cfg.inner_rtol, 1e-12) == R.ONCHIP_RTOL


def test_mesh_list_covers_both_sides_of_the_threshold():
    assert sorted(R.NODES[m[0]] for m in R.MESHES).count(R.ONCHIP_MAX_ROWS) == 6
    assert R.NODES["quad 64x64"] == 4225 > R.ONCHIP_MAX_ROWS
    assert R.NODES["quad 15x15"] == 256 and R.NODES["quad 16x15"] == 272      # last size on 256 threads, first on 1024
    for lbl in ("quad 1x1", "hex 1x1x1"):
        om, osys = R.system(lbl, R.BASE_COEFFS)
        assert len(o.boundary_nodes(om)) == om.num_nodes and not osys.rhs.any()
    om, _ = R.system("quad 2x2", R.BASE_COEFFS)
    assert om.num_nodes - len(o.boundary_nodes(om)) == 1


@pytest.mark.parametrize("label,coeffs", R.CASES, ids=IDS)
def test_restated_block_solves_match_a_direct_solve(label, coeffs):
    """(a) both blocks, with the right-hand sides the field split hands them first, against spsolve: relative 2-norm error
    within the bound that rtol 1e-12 and the block's condition number imply (block_solve_bound)."""
    _, osys = R.system(label, coeffs)
    n = osys.n
    A = osys.A.tocsr()
    A11, A22, A21 = A[:n, :n].tocsr(), A[n:, n:].tocsr(), A[n:, :n].tocsr()
    z1, its1, ok1 = R.jacobi_cg(A11, osys.rhs[:n])
    rhs2 = osys.rhs[n:] - A21 @ z1
    z2, its2, ok2 = R.jacobi_cg(A22, rhs2)
    assert ok1 and ok2
    for Ab, rhs, z, its in ((A11, osys.rhs[:n], z1, its1), (A22, rhs2, z2, its2)):
        ref = spla.spsolve(Ab.tocsc(), rhs)
        nr = np.linalg.norm(ref)
        if nr == 0.0:
            assert its == 0 and not z.any()
            continue
        err, bound = np.linalg.norm(z - ref) / nr, R.block_solve_bound(Ab)
        print(f"{label} {coeffs}: {its} iterations, error {err:.2e}, bound {bound:.2e}")
        assert err <= bound
        assert its <= Ab.shape[0]          # far from the limit 8 n + 64


def test_restated_block_solve_reports_how_it_ended():
    _, osys = R.system("hex 5x4x6", R.BASE_COEFFS)
    A11 = osys.A.tocsr()[:osys.n, :osys.n].tocsr()
    b = osys.rhs[:osys.n]
    assert R.jacobi_cg(A11, b, max_it=3)[1:] == (3, False)
    assert R.jacobi_cg(A11, np.zeros_like(b))[1:] == (0, True)
    assert R.jacobi_cg(-A11, b)[1:] == (0, False)            # p.Ap <= 0 in the first iteration
    assert R.jacobi_cg(A11, np.full_like(b, np.nan))[1:] == (0, False)
    rs = R.restated_solve("hex 5x4x6", R.BASE_COEFFS, "direct", 3)
    assert rs.stats.unconverged > 0 and rs.stats.cg_iterations == 3 * rs.stats.solves


@pytest.mark.parametrize("label,coeffs", R.CASES, ids=IDS)
def test_direct_reference_meets_its_own_residual(label, coeffs):
    """(b) a condition on the reference: the sparse direct solution has relative residual <= 1e-13, b - A x in long double."""
    _, osys = R.system(label, coeffs)
    du = (R.direct_solution(label, coeffs) - osys.u0).astype(np.longdouble)
    A = osys.A.tocsr()
    Ax = np.zeros(A.shape[0], dtype=np.longdouble)
    np.add.at(Ax, np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), A.data.astype(np.longdouble) * du[A.indices])
    r = osys.rhs.astype(np.longdouble) - Ax
    nb = np.sqrt(np.sum(osys.rhs.astype(np.longdouble) ** 2))
    if nb == 0:
        assert not r.any()
        return
    rel = float(np.sqrt(np.sum(r * r)) / nb)
    print(f"{label} {coeffs}: relative residual of the direct reference {rel:.2e}")
    assert rel <= 1e-13


def _readme_rows():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "README.md")) as f:
        text = f.read()
    rows = {}
    for line in text.splitlines():
        m = re.match(r"\| `([^`]+)` \| (direct|fieldsplit_lu) \| ([0-9.e+-]+) \| (\d+) \| (\d+) \| (\d+) \|", line)
        if m:
            rows[(m.group(1), m.group(2))] = (float(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6)))
    return rows


def table_rows():
    """The rows of the table in tests/README.md (`python tests/test_onchip_block_solve_host.py` prints them)."""
    out = []
    for label, coeffs in R.CASES:
        for preset in R.PRESETS:
            rs = R.restated_solve(label, coeffs, preset)
            err = R.rel_max_error(rs.x, R.direct_solution(label, coeffs))
            out.append((R.case_id(label, coeffs), preset, err, rs.outer_its, rs.stats.solves, rs.stats.cg_iterations))
    return out


@pytest.mark.parametrize("label,coeffs", R.CASES, ids=IDS)
def test_restated_solve_figures_are_the_ones_in_the_readme(label, coeffs):
    """(c) error against the direct solution, outer iterations and summed block CG iterations of the restated solve, both
    presets.  The table is compared with the slack the GPU tests give the device: the outer count within the restatement's
    own allowed set, +-2 CG iterations per block solve, the error within the factor 10 of another summation order (the
    BLAS kernels NumPy dispatches to differ between processors) above the floor 1e-13."""
    rows = _readme_rows()
    for preset in R.PRESETS:
        rs = R.restated_solve(label, coeffs, preset)
        assert rs.converged and rs.stats.unconverged == 0
        err = R.rel_max_error(rs.x, R.direct_solution(label, coeffs))
        terr, touter, tsolves, tcg = rows[(R.case_id(label, coeffs), preset)]
        print(f"{label} {coeffs} {preset}: error {err:.2e}, outer {rs.outer_its} {rs.outer_its_allowed}, "
              f"{rs.stats.solves} block solves, {rs.stats.cg_iterations} CG iterations")
        assert touter in rs.outer_its_allowed
        assert tsolves == 2 * (touter + 1) and rs.stats.solves == 2 * (rs.outer_its + 1)
        if touter == rs.outer_its:
            assert abs(tcg - rs.stats.cg_iterations) <= 2 * rs.stats.solves
        assert max(err, 1e-13) <= 10 * max(terr, 1e-13) and max(terr, 1e-13) <= 10 * max(err, 1e-13)


if __name__ == "__main__":
    for cid, preset, err, outer, solves, cg in table_rows():
        print(f"| `{cid}` | {preset} | {err:.1e} | {outer} | {solves} | {cg} |")
