"""p-multigrid (block pc_type pph_pmg) without a GPU: the mathematics of the cycle on the NumPy restatement
(tests/pmg_restatement.py) and the option translation."""
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
from perphil_amd.solver import degree2_unsupported, translate_options  # noqa: E402

KINDS = {"quad": R.QUAD, "tri": R.TRI, "hex": R.HEX, "tet": R.TET}


def _boundary_mask(kind, nx, ny, nz):
    m = np.zeros(R.n_nodes(kind, nx, ny, nz), bool)
    m[R.boundary_nodes(kind, nx, ny, nz)] = True
    return m


@pytest.mark.parametrize("name,size", [("quad", (6, 4, 0)), ("tri", (6, 4, 0)), ("hex", (4, 2, 3)), ("tet", (4, 2, 3))])
def test_galerkin_identity(name, size):
    """CG-1 is a subspace of CG-2 on the same affine cells: P^T A2 P is the rediscretised CG-1 operator."""
    kind = KINDS[name]
    nx, ny, nz = size
    P = PM.p_prolongation(kind, nx, ny, nz)
    K1, M1 = o.assemble_scalar(o.build_mesh(R.dim_of(kind), kind, nx, ny, nz))
    for a, c in ((1.0, 1.0), (0.01, 1.0), (1.0, 0.0)):
        A2 = PM.operator2(kind, nx, ny, nz, a, c)
        A1 = (a * K1 + c * M1).tocsr()
        err = abs(P.T @ A2 @ P - A1).max() / abs(A1).max()
        print(name, size, a, c, "galerkin", err)
        assert err <= 1e-12


# CG iterations (rtol 1e-8, random right-hand side of seed 0, homogeneous Dirichlet data on the whole boundary,
# A = a K + M) of the restatement: (kind, cells) -> (a = 1, a = 0.01)
CG_COUNTS = {
    ("quad", (16, 16, 0)): (6, 6), ("quad", (64, 64, 0)): (6, 6),
    ("tri", (16, 16, 0)): (7, 7), ("tri", (64, 64, 0)): (7, 8),
    ("hex", (8, 8, 8)): (8, 7), ("hex", (16, 16, 16)): (8, 8),
    ("tet", (8, 8, 8)): (10, 10), ("tet", (16, 16, 16)): (11, 11),
}


@pytest.mark.parametrize("name,size", list(CG_COUNTS))
def test_cg_counts(name, size):
    kind = KINDS[name]
    mask = _boundary_mask(kind, *size)
    got = []
    for a in (1.0, 0.01):
        lv = PM.build_levels(kind, *size, a, 1.0, mask)
        rhs = np.random.default_rng(0).standard_normal(mask.size)
        rhs[mask] = 0.0
        its, x = PM.pcg_iterations(lv, rhs, steps=2, rtol=1e-8)
        assert np.linalg.norm(rhs - lv[0].A @ x) <= 1e-6 * np.linalg.norm(rhs)
        got.append(its)
    print(name, size, "cg iterations", got)
    assert tuple(got) == CG_COUNTS[(name, size)]


@pytest.mark.parametrize("name,size", [("quad", (8, 8, 0)), ("tri", (8, 4, 0)), ("hex", (4, 4, 4)), ("tet", (4, 4, 4)),
                                       ("quad", (5, 3, 0)), ("tet", (3, 4, 2))])
@pytest.mark.parametrize("steps", [1, 2])
def test_cycle_is_symmetric(name, size, steps):
    kind = KINDS[name]
    mask = _boundary_mask(kind, *size)
    lv = PM.build_levels(kind, *size, 0.01, 1.0, mask)
    rng = np.random.default_rng(3)
    u, v = rng.standard_normal(mask.size), rng.standard_normal(mask.size)
    u[mask] = 0.0
    v[mask] = 0.0
    Bu, Bv = PM.cycle(lv, u, steps), PM.cycle(lv, v, steps)
    assert not Bu[mask].any() and not Bv[mask].any()
    assert abs(u @ Bv - Bu @ v) <= 1e-12 * abs(u @ Bv)
    assert u @ Bu > 0.0 and v @ Bv > 0.0


def test_option_translation():
    assert _ffi.PC_PMG == 6 and "pph_pc_apply" in _ffi.EXPORTS
    for opts, nonlinear, twin in [(spar.FIELDSPLIT_PMG_PARAMS, False, spar.FIELDSPLIT_MG_PARAMS),
                                  (spar.PICARD_PMG_SOLVER_PARAMS, True, spar.PICARD_MG_SOLVER_PARAMS)]:
        cfg, info = translate_options(opts, nonlinear=nonlinear)
        assert cfg.inner_pc_type == _ffi.PC_PMG and cfg.inner_ksp_type == _ffi.KSP_CG
        assert cfg.picard == int(nonlinear) and cfg.pc_type == _ffi.PC_FIELDSPLIT
        assert degree2_unsupported(cfg, info) is None
        # the twin differs in the block pc_type only
        assert set(opts) == set(twin)
        for k in opts:
            if k in ("fieldsplit_0", "fieldsplit_1"):
                assert opts[k] == {**twin[k], "pc_type": "pph_pmg"} and twin[k]["pc_type"] == "mg"
            else:
                assert opts[k] == twin[k]
        tcfg, _ = translate_options(twin, nonlinear=nonlinear)
        for name, _t in _ffi.SolverCfg._fields_:
            if name != "inner_pc_type":
                assert getattr(cfg, name) == getattr(tcfg, name), name
        assert tcfg.inner_pc_type == _ffi.PC_MG
    # what degree 2 refused before, it refuses still, for the same reasons
    mg = {**spar.GMRES_PARAMS, **spar._FIELDSPLIT_BASE, "fieldsplit_0": {"ksp_type": "cg", "pc_type": "mg"},
          "fieldsplit_1": {"ksp_type": "cg", "pc_type": "mg"}}
    for opts, nonlinear, word in [(spar.LINEAR_SOLVER_PARAMS, False, "preonly"), (mg, False, "mg"),
                                  (spar.FIELDSPLIT_LU_PARAMS, False, "lu"), (spar.PICARD_LU_SOLVER_PARAMS, True, "lu"),
                                  (spar.PICARD_MG_SOLVER_PARAMS, True, "mg")]:
        cfg, info = translate_options(opts, nonlinear=nonlinear)
        why = degree2_unsupported(cfg, info)
        assert why is not None and word in why
    # lu blocks and "mg" translate as before
    cfg, _ = translate_options(spar.FIELDSPLIT_LU_PARAMS)
    assert cfg.inner_pc_type == _ffi.PC_MG and cfg.inner_exact == 1
    with pytest.raises(NotImplementedError):
        translate_options({**spar.FIELDSPLIT_PMG_PARAMS, "fieldsplit_0": {"pc_type": "pph_nothing"},
                           "fieldsplit_1": {"pc_type": "pph_nothing"}})


def test_convergence_study_specs():
    names = [s.name for s in c2.pmg_solvers()]
    assert names == ["Scale-Splitting GMRES + PMG PC", "Picard + PMG"]
    assert all(c2.degree2_skip_reason(s) is None for s in c2.pmg_solvers())
    # without the flag the lists are what they were
    assert len(c2.approach_solvers()) == 5 and len(c2._default_solvers([1e-8])) == 3
    assert not any("PMG" in s.name for s in c2.approach_solvers() + c2._default_solvers([1e-8]))


def test_pmg_blocks_pass_the_degree2_gate_without_gpu():
    """A degree-2 solve with pph_pmg blocks gets past the refusals (it would need a device from there on)."""
    mesh = fd.UnitSquareMesh(4, 4, quadrilateral=True)
    V = fd.FunctionSpace(mesh, "CG", 2)
    cfg, info = translate_options(spar.PICARD_PMG_SOLVER_PARAMS, nonlinear=True)
    assert degree2_unsupported(cfg, info) is None and getattr(V, "degree", 1) == 2
