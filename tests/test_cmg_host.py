"""Coupled multigrid (pc_type pph_cmg) without a GPU: the restatement of the cycle (tests/cmg_reference.py) is pinned - its
level-0 operator, symmetry, spectrum and CG counts - together with the option translation, the refusals that must come before
any context exists, and the rejection checks: mistakes planted in the restatement have to be caught by the comparison the GPU
file uses."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cmg_reference as C  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

import perphil_amd as pa  # noqa: E402
from perphil_amd import _ffi, conditioning, convergence_2d as c2, fd, iterative_bench as ib, solver_parameters as spar  # noqa: E402
from perphil_amd.solver import degree2_unsupported, translate_options  # noqa: E402

R = C.R
KINDS = {"quad": C.QUAD, "tri": C.TRI, "hex": C.HEX, "tet": C.TET}

# (mesh, beta, k2) -> (kappa(B A), CG iterations to 1e-8): the measured values of the feature's issue (2 steps per side)
TABLE = {
    ("quad", (16, 16, 0), 1.0, 0.01): (1.10, 6), ("quad", (16, 16, 0), 1e2, 0.01): (1.79, 10), ("quad", (16, 16, 0), 1e4, 0.01): (2.57, 13),
    ("tri", (12, 12, 0), 1.0, 0.01): (1.23, 7), ("tri", (12, 12, 0), 1e2, 0.01): (1.48, 9), ("tri", (12, 12, 0), 1e4, 0.01): (1.54, 9),
    ("hex", (8, 8, 8), 1.0, 0.01): (1.13, 6), ("hex", (8, 8, 8), 1e4, 0.01): (5.85, 20),
    ("tet", (4, 4, 4), 1e2, 0.01): (1.73, 9),
    ("quad", (16, 16, 0), 1e2, 1.0): (1.10, 5),
}


def _levels(name, size, beta, k2=C.K2, mixed=False, **kw):
    kind = KINDS[name]
    n = R.level_nodes(kind, *size)[0]
    masks = C.masks_from_nodes(n, C.mixed_nodes(kind, *size)) if mixed else C.boundary_masks(kind, *size)
    return C.coupled_hierarchy(kind, *size, masks, k2=k2, beta=beta, **kw)


@pytest.mark.parametrize("name,size", [("quad", (8, 6, 0)), ("tri", (6, 4, 0)), ("hex", (4, 4, 2)), ("tet", (2, 4, 4))])
@pytest.mark.parametrize("mixed", [False, True])
def test_level0_is_the_monolithic_matrix(name, size, mixed):
    kind = KINDS[name]
    lv = _levels(name, size, 1e2, mixed=mixed)
    om = o.build_mesh(R.dim_of(kind), kind, *size)
    osys = o.build_system(om, o.Params(k1=C.K1, k2=C.K2, beta=1e2, mu=C.MU), mms=False, mask1=lv[0].mask[0], mask2=lv[0].mask[1])
    assert abs(lv[0].A - osys.A).max() <= 1e-14 * abs(osys.A).max()
    if mixed:
        assert (lv[0].mask[0] != lv[0].mask[1]).any()


@pytest.mark.parametrize("name,size", [("quad", (16, 12, 0)), ("tri", (8, 8, 0)), ("hex", (4, 4, 8)), ("tet", (4, 4, 4))])
def test_diagonal_blocks_are_the_oracle_hierarchy(name, size):
    """Levels, masks, diagonal blocks, scalar bounds and transfers are dpp_mg_oracle.build_hierarchy's, field by field."""
    kind = KINDS[name]
    lv = _levels(name, size, 1e2, mixed=True)
    for f, coefK in enumerate((C.K1 / C.MU, C.K2 / C.MU)):
        ref = C.G.build_hierarchy(R.dim_of(kind), kind, *size, coefK, 1e2 / C.MU, lv[0].mask[f])
        assert len(ref) == len(lv) and len(lv) >= 2
        for L, g in zip(lv, ref):
            n = L.n
            blk = L.A[:n, :n] if f == 0 else L.A[n:, n:]
            assert np.array_equal(L.mask[f], g.mask) and abs(blk - g.A).max() == 0.0
            assert (L.P is None) == (g.P is None) and (g.P is None or abs(L.P - g.P).max() == 0.0)
        assert all(L.lam_scalar >= g.lam for L, g in zip(lv, ref))


@pytest.mark.parametrize("key", list(TABLE), ids=lambda k: f"{k[0]}-{k[1][0]}-beta{k[2]:g}-k2_{k[3]:g}")
def test_spectrum_and_cg_counts(key):
    name, size, beta, k2 = key
    kappa_max, its_max = TABLE[key]
    lv = _levels(name, size, beta, k2)
    ev, B = C.ba_spectrum(lv, 2)
    sym = abs(B - B.T).max() / abs(B).max()
    rhs = C._masked(np.random.default_rng(0).standard_normal(2 * lv[0].n), lv[0].mask)
    x, its, conv = C.cg_count(lv, rhs)
    print(key, "symmetry", sym, "lambda_max", ev.max(), "kappa", ev.max() / ev.min(), "cg", its)
    assert sym <= 1e-12
    assert ev.min() > 0.0 and ev.max() <= 1.0 + 1e-12
    assert ev.max() / ev.min() <= kappa_max * 1.01
    assert conv and its <= its_max
    assert np.linalg.norm(rhs - lv[0].A @ x) <= 1e-6 * np.linalg.norm(rhs)


def test_the_sweep_the_feature_replaces_stalls():
    """rho(A11^-1 A12 A22^-1 A21) at beta = 1e2 on quad 16 x 16: a fixed-stress sweep contracts by 0.83 only."""
    rho = C.sweep_contraction(_levels("quad", (16, 16, 0), 1e2))
    print("sweep contraction", rho)
    assert 0.8 < rho < 1.0
    assert C.sweep_contraction(_levels("quad", (16, 16, 0), 1.0)) < 0.05


def test_cycle_with_different_masks_is_symmetric_and_zero_on_constrained_dofs():
    for name, size in (("quad", (8, 8, 0)), ("hex", (4, 4, 4)), ("quad", (5, 5, 0))):
        lv = _levels(name, size, 1e2, mixed=True)
        rng = np.random.default_rng(3)
        u, v = rng.standard_normal(2 * lv[0].n), rng.standard_normal(2 * lv[0].n)
        m = np.concatenate(lv[0].mask)
        Bu, Bv = C.apply_reference(lv, u, 2), C.apply_reference(lv, v, 2)
        assert not Bu[m].any() and not Bv[m].any()
        u[m] = v[m] = 0.0
        assert abs(u @ Bv - Bu @ v) <= 1e-12 * abs(u @ Bv)
        assert u @ Bu > 0.0 and v @ Bv > 0.0


def test_determinant_formula_survives_the_cancellation():
    """d11 d22 - d12^2 loses every digit once beta M_ii dominates; s1 s2 - d12 (s1 + s2) does not."""
    kd, md, b = 2.0 + 2.0 / 3.0, 1.7e-3, 1e12
    d11, d22, d12 = 1.0 * kd + b * md, 0.01 * kd + b * md, -b * md
    i11, i12, i22 = C.block_inverse(np.array([d11]), np.array([d22]), np.array([d12]))
    ld = np.longdouble
    det = (ld(d11) + ld(d12)) * (ld(d22) + ld(d12)) - ld(d12) * ((ld(d11) + ld(d12)) + (ld(d22) + ld(d12)))
    assert abs(i11[0] * float(det) / d22 - 1.0) <= 1e-12
    # the plain form rounds two products of size 2.9e18 to get 4.6e9: an error of the order eps d11 d22 / det = 7e-8
    assert abs((d11 * d22 - d12 * d12) / float(det) - 1.0) > 1e-9


def test_longdouble_restatement_agrees():
    lv = _levels("quad", (16, 12, 0), 1e4, mixed=True)
    lq = C.levels_as(lv, np.longdouble)
    for name, r in C.probe_vectors(lv, 5):
        d = C.rel_err(C.apply_reference(lv, r, 2), C.apply_reference(lq, r, 2).astype(np.float64))
        print(name, "float64 against longdouble", d)
        assert d <= 1e-11


@pytest.mark.parametrize("name,size", [("quad", (16, 12, 0)), ("hex", (8, 8, 8))])
def test_planted_mistakes_are_caught(name, size):
    """Dropping the coupling from D_l, taking lam from the scalar rule and ignoring one field's mask on a coarse level each
    miss CYCLE_BOUND - by the comparison of test_cmg_gpu.py - so a device cycle that made one of them would fail there."""
    good = _levels(name, size, 1e2, mixed=True)
    vectors = C.probe_vectors(good, 7)
    ref = lambda r: C.apply_reference(good, r, 2)   # noqa: E731
    assert R.worst_error(ref, ref, vectors)[0] == 0.0
    for what, bad, kw in (("D_1 without the coupling", _levels(name, size, 1e2, mixed=True, drop_coupling=1), {}),
                          ("D_0 without the coupling", _levels(name, size, 1e2, mixed=True, drop_coupling=0), {}),
                          ("lam_1 from the scalar rule", _levels(name, size, 1e2, mixed=True, scalar_lam=1), {}),
                          ("lam_0 from the scalar rule", _levels(name, size, 1e2, mixed=True, scalar_lam=0), {}),
                          ("field 1's mask ignored on level 1", good, {"ignore_mask": (1, 1)}),
                          ("field 0's mask ignored on level 1", good, {"ignore_mask": (1, 0)})):
        w, at, _ = R.worst_error(lambda r: C.apply_reference(bad, r, 2, **kw), ref, vectors)
        print(name, what, "worst error", w, "at", at)
        assert w > 100 * C.CYCLE_BOUND, what


def test_launch_rule():
    assert C.cmg_lanes(C.HEX) == 8 and C.cmg_lanes(C.TET) == 8 and C.cmg_lanes(C.QUAD) == 4 and C.cmg_lanes(C.TRI) == 4
    assert C.rows_per_pass(C.HEX) == 65536 and C.rows_per_pass(C.QUAD) == 131072
    assert not C.row_kernel_loops(C.HEX, 40 ** 3) and C.row_kernel_loops(C.HEX, 41 ** 3)
    assert not C.row_kernel_loops(C.QUAD, 362 ** 2) and C.row_kernel_loops(C.QUAD, 363 ** 2)
    assert not C.node_kernel_loops(512 ** 2) and C.node_kernel_loops(513 ** 2)


def test_option_translation():
    assert _ffi.PC_CMG == 7 and "pph_pc_apply_coupled" in _ffi.EXPORTS
    cfg, info = translate_options(spar.CG_CMG_PARAMS)
    assert cfg.pc_type == _ffi.PC_CMG and cfg.ksp_type == _ffi.KSP_CG and cfg.picard == 0
    assert cfg.rtol == 1e-8 and cfg.atol == 1e-12 and cfg.mg_smooth == 2
    cfg, _ = translate_options({**spar.CG_CMG_PARAMS, "pph_mg_smooth": 3})
    assert cfg.mg_smooth == 3
    cfg, _ = translate_options(spar.GMRES_CMG_PARAMS)
    assert cfg.pc_type == _ffi.PC_CMG and cfg.ksp_type == _ffi.KSP_GMRES
    # the monolithic twins differ in pc_type only
    tcfg, _ = translate_options(spar.CG_BLOCK_JACOBI_PARAMS)
    for name, _t in _ffi.SolverCfg._fields_:
        if name != "pc_type":
            assert getattr(translate_options(spar.CG_CMG_PARAMS)[0], name) == getattr(tcfg, name), name
    assert degree2_unsupported(*translate_options(spar.CG_CMG_PARAMS)) is not None
    # the scalar cycle is refused on the monolithic operator as before
    with pytest.raises(NotImplementedError):
        translate_options({**spar.GMRES_PARAMS, "pc_type": "mg"})
    with pytest.raises(NotImplementedError):
        translate_options({**spar.GMRES_PARAMS, "pc_type": "pph_pmg"})


def _problem(nx=4, degree=1, cube=False):
    mesh = fd.UnitCubeMesh(nx, nx, nx, hexahedral=True) if cube else pa.create_mesh(nx, nx, quadrilateral=True)
    V = fd.FunctionSpace(mesh, "CG", degree)
    W = V * V
    params = pa.DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
    bcs = [fd.DirichletBC(W.sub(0), fd.Constant(0.0), "on_boundary"), fd.DirichletBC(W.sub(1), fd.Constant(0.0), "on_boundary")]
    return mesh, V, W, params, bcs


def _no_context(mesh):
    return mesh._ctx is None and not mesh.__dict__.get("_ctx_deg")


def test_refusals_come_before_any_context():
    # degree 2
    mesh, _V, W, params, bcs = _problem(degree=2)
    for opts in (spar.CG_CMG_PARAMS, spar.GMRES_CMG_PARAMS):
        with pytest.raises(NotImplementedError, match="pph_cmg"):
            pa.solve_dpp(W, params, bcs, opts)
    a, _ = pa.dpp_form(W, params)
    with pytest.raises(NotImplementedError, match="pph_cmg"):
        conditioning.preconditioned_condition_number(a, bcs, "pph_cmg")
    with pytest.raises(NotImplementedError, match="pph_cmg"):
        conditioning.effective_condition_numbers(W, params, bcs, spar.CG_CMG_PARAMS)
    assert _no_context(mesh)
    # a distributed mesh
    mesh, _V, W, params, bcs = _problem(cube=True)
    from perphil_amd.partition import make_slab

    mesh._decided, mesh._slab = True, make_slab(mesh.nx, mesh.ny, mesh.nz, 2, 0)   # (what fd.Mesh decides under two ranks)
    assert mesh.distributed
    with pytest.raises(NotImplementedError, match="distributed"):
        pa.solve_dpp(W, params, bcs, spar.CG_CMG_PARAMS)
    assert _no_context(mesh)
    # as a block preconditioner
    mesh, V, W, params, bcs = _problem()
    block = {"ksp_type": "cg", "pc_type": "pph_cmg"}
    for opts, solve in (({**spar.GMRES_PARAMS, **spar._FIELDSPLIT_BASE, "fieldsplit_0": block, "fieldsplit_1": block}, pa.solve_dpp),
                        ({**spar._PICARD_BASE, **spar._FIELDSPLIT_BASE, "fieldsplit_0": block, "fieldsplit_1": block},
                         pa.solve_dpp_nonlinear)):
        with pytest.raises(NotImplementedError, match="pph_cmg"):
            solve(W, params, bcs, opts)
    # on a scalar block
    (am, _), (ai, _) = pa.dpp_delayed_form(V, V, params, fd.Function(V), fd.Function(V))
    for form, b in ((am, [bcs[0]]), (ai, [bcs[1]])):
        with pytest.raises(NotImplementedError, match="scalar block"):
            conditioning.preconditioned_condition_number(form, b, "pph_cmg")
    # every pairing refused before stays refused
    a, _ = pa.dpp_form(W, params)
    for form, b, pc in ((a, bcs, "mg"), (a, bcs, "pph_pmg"), (am, [bcs[0]], "pph_block2"), (a, bcs, "fieldsplit"), (a, bcs, "none")):
        with pytest.raises(NotImplementedError):
            conditioning.preconditioned_condition_number(form, b, pc)
    assert _no_context(mesh)


def test_opt_in_specs_leave_the_defaults_alone():
    names = [s.name for s in c2.cmg_solvers()]
    assert names == ["CG + coupled MG"]
    assert c2.degree2_skip_reason(c2.cmg_solvers()[0]) is not None
    assert len(c2.approach_solvers()) == 5 and len(c2._default_solvers([1e-8])) == 3
    assert not any("coupled" in s.name for s in c2.approach_solvers() + c2._default_solvers([1e-8]) + c2.pmg_solvers())
    assert [s[0] for s in ib.cmg_configurations()] == ["CG + coupled MG"]
    assert not any("coupled" in s[0] for s in ib.default_configurations())
