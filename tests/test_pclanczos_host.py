"""CPU checks behind the preconditioned Lanczos path (pph_preconditioned_extremes, pph_eig.hip): the NumPy restatement of
the iteration (pclanczos_reference.py) against dense eigenvalues of C^T B C (A_ff = C C^T, B built column by column) under
Jacobi and under the oracle's V-cycle, the closed form of the Jacobi-scaled mass matrix, the sign rule, the launch rule, and
the parts of the feature that need no device: the declared and exported symbol and the refusals of the public API, which
are raised before any context exists."""
import ctypes
import os
import re

import numpy as np
import pytest

import lanczos_reference as lr
import pclanczos_reference as pr
from oracle import dpp_mg_oracle as mg
from oracle import dpp_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K1, K2, BETA, MU = 1.0, 0.01, 3.0, 2.0
MESHES = {"quad": (2, o.CELL_QUAD, (16, 12, 0)), "tri": (2, o.CELL_TRI, (12, 8, 0)), "hex": (3, o.CELL_HEX, (8, 4, 6)),
          "tet": (3, o.CELL_TET, (4, 4, 4))}


def _masks(mesh):
    """Field 0 constrained on the whole boundary, field 1 on the side x = 0 only."""
    X = mesh.coords
    m0 = np.zeros(len(X), dtype=bool)
    m0[o.boundary_nodes(mesh)] = True
    return m0, np.abs(X[:, 0]) < 1e-12


@pytest.fixture(scope="module")
def hierarchies():
    """name -> per field (levels, mask): built once, read by every test of this module."""
    out = {}
    for name, (dim, kind, cells) in MESHES.items():
        mesh = o.build_mesh(dim, kind, *cells)
        out[name] = [(mg.build_hierarchy(dim, kind, *cells, ck / MU, BETA / MU, mask), mask)
                     for ck, mask in zip((K1, K2), _masks(mesh))]
    return out


def _check_against_dense(A, apply_B, mask, what):
    free = np.nonzero(~mask)[0]
    ref = pr.dense_pencil(A, pr.dense_operator(apply_B, A.shape[0], free), free)
    r = pr.pc_lanczos_extremes(A, apply_B, mask, tol=1e-10)
    errs = [abs(r["lambda_min"] / ref["lambda_min"] - 1), abs(r["lambda_max"] / ref["lambda_max"] - 1)]
    print(f"{what}: steps {r['iterations']} lambda {ref['lambda_min']:.6f} {ref['lambda_max']:.6f} rel. errors "
          f"{errs[0]:.2e} {errs[1]:.2e} a {ref['a']:.2e}")
    assert r["converged"] == 1 and r["breakdown"] == 0, (what, r)
    assert max(errs) <= 1e-9, (what, r, ref)
    return r, ref


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", list(MESHES))
def test_restatement_matches_dense_eigenvalues_under_jacobi(hierarchies, name, field):
    levels, mask = hierarchies[name][field]
    lv = levels[0]
    _check_against_dense(lv.A, lambda r: lv.dinv * r, mask, f"{name} field {field} jacobi")


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", list(MESHES))
def test_restatement_matches_dense_eigenvalues_under_the_vcycle(hierarchies, name, field):
    """V(2,2) of oracle/dpp_mg_oracle.py.  tol 1e-10 is reached on these meshes (a few hundred rows: the clustered upper
    end is resolved once the Krylov space is a good part of the whole space); the spectrum lies in about [0.9, 1]."""
    levels, mask = hierarchies[name][field]
    assert len(levels) >= 2
    r, ref = _check_against_dense(levels[0].A, lambda b: mg.vcycle(levels, b, 2), mask, f"{name} field {field} V(2,2)")
    assert ref["a"] <= 1e-12 and 0.5 < ref["lambda_min"] < ref["lambda_max"] < 1.0 + 1e-9


@pytest.mark.parametrize("cells", [(20, 20, 20), (33, 32, 31), (48, 48, 48)])
def test_scaled_mass_matrix_closed_form(cells):
    """D^-1 M on a box of hexes: (1/8, 27/8) exactly - the 1D pencils (M_1, diag M_1) have the extremes 1/2 and 3/2 for
    every cell count (eigenvectors (-1)^i and 1)."""
    lo, hi = pr.box_scaled_mass_extremes(cells)
    assert abs(lo - 0.125) <= 2e-15 and abs(hi - 3.375) <= 2e-15, (lo, hi)


def test_restatement_reproduces_the_scaled_mass_closed_form():
    cells = (7, 5, 6)
    _, M = o.assemble_scalar(o.build_mesh(3, o.CELL_HEX, *cells))
    M = M.tocsr()
    d = 1.0 / M.diagonal()
    r = pr.pc_lanczos_extremes(M, lambda x: d * x, None, tol=1e-10)
    want = pr.box_scaled_mass_extremes(cells)
    assert r["converged"] == 1
    assert r["lambda_min"] == pytest.approx(want[0], rel=1e-9) and r["lambda_max"] == pytest.approx(want[1], rel=1e-9)
    assert r["kappa"] == pytest.approx(27.0, rel=1e-9)


def test_a_negative_preconditioner_is_refused_not_reported_as_a_breakdown(hierarchies):
    levels, mask = hierarchies["quad"][0]
    lv = levels[0]
    with pytest.raises(pr.NotPositiveDefinite, match="start"):
        pr.pc_lanczos_extremes(lv.A, lambda r: -lv.dinv * r, mask)
    # indefinite on the Krylov space, positive on the start vector: caught by the scan of r.Br at a step
    n = lv.A.shape[0]
    u0 = lr.start_vector(n)
    u0[mask] = 0.0
    sign = np.ones(n)
    free = np.nonzero(~mask)[0]
    sign[free[np.argsort(np.abs(u0[free]))[: len(free) // 2]]] = -1.0   # negative where the start vector is small
    assert u0 @ (sign * lv.dinv * u0) > 0.0
    with pytest.raises(pr.NotPositiveDefinite, match="step"):
        pr.pc_lanczos_extremes(lv.A, lambda r: sign * lv.dinv * r, mask, tol=1e-10)


def test_no_free_rows_is_refused():
    s = o.build_system(o.build_mesh(2, o.CELL_QUAD, 1, 1), o.Params(), mms=False)
    A = s.A.tocsr()[: s.n, : s.n]
    with pytest.raises(ValueError, match="no free rows"):
        pr.pc_lanczos_extremes(A, lambda r: r, np.ones(s.n, dtype=bool))


def test_launch_rule():
    """min(ceil(ceil(n / 2) / 256), 1024) blocks of 256 threads on pairs of rows: one pass up to GRID_CAPACITY_ROWS rows."""
    assert pr.GRID_CAPACITY_ROWS == lr.GRID_CAPACITY_ROWS == 1024 * 256 * 2
    for n, blocks in ((1, 1), (2, 1), (512, 1), (513, 2), (221, 1), (524288, 1024), (524289, 1024), (81 ** 3, 1024)):
        assert pr.grid_blocks(n) == blocks, n
    assert 81 ** 3 > pr.GRID_CAPACITY_ROWS and (81 ** 3) % 2 == 1


def test_defaults_differ_from_the_plain_entry_point():
    import inspect

    from perphil_amd import _ffi, conditioning

    d = {k: v.default for k, v in inspect.signature(_ffi.Context.preconditioned_extremes).parameters.items()}
    assert (d["mg_smooth"], d["tol"], d["max_it"], d["check_every"]) == (2, pr.DEFAULT_TOL, pr.DEFAULT_MAX_IT, pr.DEFAULT_CHECK_EVERY)
    d = {k: v.default for k, v in inspect.signature(conditioning.preconditioned_condition_number).parameters.items()}
    assert (d["mg_smooth"], d["tol"]) == (2, 1e-4)
    d = {k: v.default for k, v in inspect.signature(conditioning.effective_condition_numbers).parameters.items()}
    assert (d["nonlinear"], d["tol"]) == (False, 1e-4)


# ---- fail without the feature -----------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    from perphil_amd import _ffi

    with open(os.path.join(ROOT, "include", "perphil_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+pph_preconditioned_extremes\s*\(\s*pph_ctx\s*\*\s*ctx,\s*int which,\s*int pc_type,\s*int mg_smooth,"
                     r"\s*double tol,\s*int max_it,\s*int check_every,\s*double\s*\*\s*out", header)
    assert "pph_preconditioned_extremes" in _ffi.EXPORTS
    fn = getattr(_ffi.lib, "pph_preconditioned_extremes")
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8


def _forms(nx=4, degree=1):
    import perphil_amd as pa
    from perphil_amd import fd

    mesh = pa.create_mesh(nx, nx, quadrilateral=True)
    V = fd.FunctionSpace(mesh, "CG", degree)
    W = V * V
    params = pa.DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
    a, _ = pa.dpp_form(W, params)
    (am, _), (ai, _) = pa.dpp_delayed_form(V, V, params, fd.Function(V), fd.Function(V))
    bcs = [fd.DirichletBC(W.sub(0), fd.Constant(0.0), "on_boundary"), fd.DirichletBC(W.sub(1), fd.Constant(0.0), "on_boundary")]
    return mesh, W, params, a, am, ai, bcs


def _no_context(mesh):
    return mesh._ctx is None and not mesh.__dict__.get("_ctx_deg")


def test_public_api_refuses_before_any_context_exists():
    from perphil_amd import conditioning

    mesh, _W, _params, a, am, ai, bcs = _forms()
    for form, b, pc in ((a, bcs, "fieldsplit"), (am, [bcs[0]], "fieldsplit"), (a, bcs, "none"), (ai, [bcs[1]], "none"),
                        (a, bcs, "mg"), (a, bcs, "pph_pmg"), (am, [bcs[0]], "pph_block2"), (a, bcs, "lu")):
        with pytest.raises(NotImplementedError):
            conditioning.preconditioned_condition_number(form, b, pc)
    assert _no_context(mesh)
    mesh2, _W2, _p2, _a2, am2, ai2, bcs2 = _forms(degree=2)
    for form, b in ((am2, [bcs2[0]]), (ai2, [bcs2[1]])):
        with pytest.raises(NotImplementedError, match="pph_pmg"):
            conditioning.preconditioned_condition_number(form, b, "mg")
    assert _no_context(mesh2)


def test_exact_blocks_have_condition_number_one_without_a_context():
    from perphil_amd import conditioning
    from perphil_amd import solver_parameters as sp

    mesh, W, params, _a, _am, _ai, bcs = _forms()
    assert conditioning.effective_condition_numbers(W, params, bcs, sp.LINEAR_SOLVER_PARAMS) == {"macro": 1.0, "micro": 1.0}
    assert conditioning.effective_condition_numbers(W, params, bcs, sp.PICARD_LU_SOLVER_PARAMS, nonlinear=True) == {"macro": 1.0, "micro": 1.0}
    assert conditioning.effective_condition_numbers(W, params, bcs, sp.FIELDSPLIT_LU_PARAMS) == {"macro": 1.0, "micro": 1.0}
    for opts in (sp.PLAIN_GMRES_PARAMS, sp.FIELDSPLIT_GMRES_PARAMS):   # pc_type none, monolithic and per block
        with pytest.raises(NotImplementedError):
            conditioning.effective_condition_numbers(W, params, bcs, opts)
    assert _no_context(mesh)
