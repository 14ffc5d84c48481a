"""Self-checks of the references of tests/test_mg_cycle_gpu.py (tests/mg_cycle_reference.py) and the sensitivity of its
comparisons: the restated cycle is the oracle's bit for bit, the matrix-free hierarchy equals the SciPy one to rounding,
the restated launch rules give the branches the GPU cases claim, and every comparison REJECTS a reference-built stand-in
for device output that is wrong by a little (one transfer weight, one dropped mask, the neighbouring level's smoother
weight, a loose coarsest solve, a skipped post-smoothing, r.z of the first PCG iteration)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mg_cycle_reference as MC  # noqa: E402
from oracle import dpp_mg_oracle as G  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

K1, K2, BETA, MU = MC.K1, MC.K2, MC.BETA, MC.MU
COEF_K = (K1 / MU, K2 / MU)
EPS = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def _hier(kind, nx, ny, nz, which, variant=0, matfree=False):
    """(levels, dims, mask) of block `which`, built once per module."""
    n = MC.level_nodes(kind, nx, ny, nz)[0]
    mask = MC.mask_of(n, MC.dirichlet_nodes(kind, nx, ny, nz, variant, which))
    build = MC.matfree_hierarchy if matfree else (lambda k, *a: G.build_hierarchy(MC.dim_of(k), k, *a))
    return build(kind, nx, ny, nz, COEF_K[which], BETA / MU, mask), MC.level_dims(kind, nx, ny, nz), mask


def test_restated_cycle_is_the_oracle_cycle():
    for kind, nx, ny, nz in [(MC.QUAD, 8, 12, 0), (MC.TRI, 8, 8, 0), (MC.HEX, 4, 8, 4), (MC.TET, 4, 4, 8)]:
        lv, _, mask = _hier(kind, nx, ny, nz, 1)
        assert len(lv) == len(MC.level_nodes(kind, nx, ny, nz)) >= 2
        assert [l.mask.size for l in lv] == MC.level_nodes(kind, nx, ny, nz)
        r = np.random.default_rng(3).standard_normal(mask.size)
        r[mask] = 0.0
        for steps in (1, 2):
            assert np.array_equal(MC.apply_reference(lv, r, steps), G.vcycle(lv, r, steps))
        for k in (1, 2, 3):
            prec = lambda v: G.vcycle(lv, v, 1)   # noqa: E731
            assert np.array_equal(MC.pcg_fixed(lv[0].A, r, prec, k), o.pcg(lv[0].A, r, prec, norm="none", max_it=k).x)
    # a mesh that cannot be coarsened: max(steps, 2) Chebyshev steps
    lv, _, mask = _hier(MC.HEX, 3, 4, 2, 0)
    assert len(lv) == 1
    r = np.where(mask, 0.0, 1.0)
    assert np.array_equal(MC.apply_reference(lv, r, 1), G.chebyshev(lv[0], r, None, 2))
    assert np.array_equal(MC.apply_reference(lv, r, 3), G.chebyshev(lv[0], r, None, 3))


def test_restated_launch_rules():
    """The branches the GPU cases rely on, from the restated rules of pph_mg.hip."""
    b = MC.branch_of(MC.QUAD, 1024, 1024)
    assert b["levels"][-5:] == [1089, 289, 81, 25, 9] and b["NL"] == 4 and b["lt"] == len(b["levels"]) - 4
    assert MC.branch_of(MC.HEX, 16, 16, 16) == {"levels": [4913, 729, 125, 27], "nlev": 4, "lt": 1, "NL": 3,
                                                 "coarsest": "tail, one-wave CG"}
    b = MC.branch_of(MC.HEX, 20, 20, 20)
    assert b["levels"] == [9261, 1331, 216] and b["NL"] == 1 and b["coarsest"] == "tail, workgroup CG"
    assert MC.branch_of(MC.HEX, 12, 8, 16)["levels"] == [1989, 315, 60]
    assert MC.branch_of(MC.QUAD, 40, 36)["levels"] == [1517, 399, 110] and MC.branch_of(MC.QUAD, 40, 36)["NL"] == 2
    # option mg_tail_rows moves the first tail level; 0: no tail; coarse_on_device 0: host-driven CG
    got = {rows: MC.branch_of(MC.QUAD, 64, 64, 0, rows)["NL"] for rows in (5000, 100, 30, 10, 0)}
    assert got == {5000: 4, 100: 3, 30: 2, 10: 1, 0: 0}
    assert MC.branch_of(MC.QUAD, 64, 64, 0, 0)["coarsest"] == "k_coarse_cg_sell"
    assert MC.branch_of(MC.QUAD, 64, 64, 0, 5000, False)["coarsest"] == "pph_cg_jacobi"
    # 3D: NL = 4 needs a first tail level of <= 1024 nodes whose cells halve three more times (multiples of 8, >= 16 per
    # direction): the smallest such level has 17^3 = 4913 nodes
    for kind in (MC.HEX, MC.TET):
        best = 0
        for c in range(2, 40):
            ns = MC.level_nodes(kind, c, c, c)
            best = max(best, len(ns) - MC.tail_begin(ns, kind))
        assert best == 3
        assert min((8 * a + 1) * (8 * b + 1) * (8 * c + 1) for a in (2, 3) for b in (2, 3) for c in (2, 3)) > MC.MG_TAIL_ROWS
    # the LDS pool of the operators limits the tail before the row cap does: tets 8 x 8 x 60
    assert MC.tail_lds([729, 125, 27], 27) > 0 and MC.tail_lds([1025], 27) == 0 and MC.tail_lds([900, 300], 27) == 0
    # grid-stride loops
    assert MC.mg_grid(1) == 1 and MC.mg_grid(10 ** 7) == 2048 and not MC.loops(524288) and MC.loops(524289)
    d = MC.level_dims(MC.HEX, 160, 160, 160)
    assert MC.loops(MC.q1_pairs(d[0])) and MC.loops(d[1][0] ** 3) and d[1][0] ** 3 == 531441
    d = MC.level_dims(MC.QUAD, 1024, 1024)
    assert MC.loops(MC.q1_pairs(d[0])) and d[0][0] * d[0][1] > 1048576


MATFREE_CASES = [(MC.QUAD, 8, 12, 0, 0), (MC.QUAD, 40, 36, 0, 0), (MC.QUAD, 16, 16, 0, 1), (MC.HEX, 12, 8, 16, 0),
                 (MC.HEX, 8, 8, 8, 1), (MC.HEX, 4, 6, 10, 0)]


@pytest.mark.parametrize("kind,nx,ny,nz,variant", MATFREE_CASES)
def test_matrix_free_hierarchy_equals_the_scipy_oracle(kind, nx, ny, nz, variant):
    """Operators, diagonals, masks, bounds, transfers and one cycle: the differences are bounded by 100 x what the SciPy
    oracle differs from itself under a permuted numbering (at least one unit of rounding, which such a drift cannot
    resolve below)."""
    for which in (0, 1):
        lv, _, mask = _hier(kind, nx, ny, nz, which, variant)
        mf, _, _ = _hier(kind, nx, ny, nz, which, variant, True)
        pl, perm = MC.permuted(lv, 7)
        rng = np.random.default_rng(11)
        assert len(lv) == len(mf)
        for l, (a, b, p) in enumerate(zip(lv, mf, pl)):
            assert np.array_equal(a.mask, b.mask)
            x = rng.standard_normal(a.mask.size)
            y = a.A @ x
            # drift of the bound: the rows of the permuted SciPy level are summed in another order
            rows_p = np.asarray(abs(p.A).sum(axis=1)).ravel() * p.dinv
            lam_p = float(rows_p.max())
            d_lam = max(abs(lam_p - a.lam) / a.lam, EPS)
            e_lam = abs(b.lam - a.lam) / a.lam
            scale = abs(y).max()
            d_A = EPS   # a row of <= 27 products: one unit of rounding is what a reordering moves
            e_A = abs(b.A @ x - y).max() / scale
            e_d = abs(b.dinv - a.dinv).max() / abs(a.dinv).max()
            print(f"{MC.KIND_NAME[kind]} {nx}x{ny}x{nz} block {which} level {l}: lam {a.lam:.15f} diff {e_lam:.1e} (drift {d_lam:.1e}), "
                  f"A x diff {e_A:.1e}, dinv diff {e_d:.1e}")
            assert e_lam <= 100 * d_lam and e_A <= 100 * d_A and e_d <= 100 * EPS
            if a.P is not None:
                e = rng.standard_normal(a.P.shape[1])
                assert abs(b.P @ e - a.P @ e).max() <= 100 * EPS * abs(e).max()
                assert abs(b.P.T @ x - a.P.T @ x).max() <= 100 * EPS * abs(a.P.T @ x).max()
        for steps in (1, 2):
            for name, r in MC.probe_vectors(lv, 5):
                ref = MC.apply_reference(lv, r, steps)
                drift = max(MC.rel_err(MC.apply_permuted(pl, perm, r, steps), ref), EPS)
                err = MC.rel_err(MC.apply_reference(mf, r, steps), ref)
                print(f"   steps {steps} {name}: matrix-free against SciPy {err:.2e}, SciPy permuted against itself {drift:.2e}")
                assert err <= 100 * drift


# ---------------------------------------------------------------------------------------------------------------------
# the comparisons of part 1 must reject wrong cycles
# ---------------------------------------------------------------------------------------------------------------------
REJECT_MESHES = [(MC.HEX, 16, 16, 16), (MC.HEX, 20, 20, 20), (MC.TRI, 32, 32, 0), (MC.QUAD, 40, 36, 0), (MC.TET, 8, 8, 8),
                 (MC.TET, 12, 12, 12)]


def _rejected(lv, steps, wrong, vectors):
    worst, name, _ = MC.worst_error(wrong, lambda r: MC.apply_reference(lv, r, steps), vectors)
    return worst, name


@pytest.mark.parametrize("kind,nx,ny,nz", REJECT_MESHES)
def test_cycle_comparison_rejects_wrong_cycles(kind, nx, ny, nz):
    for which in (0, 1):
        lv, dims, mask = _hier(kind, nx, ny, nz, which)
        nlev = len(lv)
        vectors = MC.probe_vectors(lv, 17)
        assert len(vectors) == nlev
        for steps in (1, 2):
            stand_ins = {}
            for l in range(nlev - 1):
                # (a coarse level with one or two free nodes - 3^3 under 16^3 hexahedra - carries so little of z that a weight
                # off by 1e-6 moves z by 5e-12; a weight wrong by a factor moves it by 1e-6 and more.  Said in tests/README.md)
                if int((~lv[l + 1].mask).sum()) >= 20:
                    wl = MC.with_transfer_weight(lv, dims, l, 1e-6)
                    stand_ins[f"transfer weight x (1 + 1e-6) between levels {l} and {l + 1}"] = \
                        lambda r, wl=wl: MC.apply_reference(wl, r, steps)
                stand_ins[f"smoother weight of level {l + 1} on level {l}"] = \
                    lambda r, l=l: MC.apply_reference(lv, r, steps, lam_from_next=l)
            for l in range(1, nlev):
                stand_ins[f"mask of level {l} dropped"] = lambda r, l=l: MC.apply_reference(lv, r, steps, drop_mask=l)
            for l in range(1, nlev - 1):
                stand_ins[f"no post-smoothing on level {l}"] = lambda r, l=l: MC.apply_reference(lv, r, steps, skip_post=l)
            # (a coarsest level with a handful of free nodes is solved exactly by as many CG iterations at any tolerance:
            # 16^3 hexahedra end at 3^3 nodes, one of them free)
            if int((~lv[-1].mask).sum()) >= 20:
                stand_ins["coarsest solve stopped at rtol 1e-6"] = lambda r: MC.apply_reference(lv, r, steps, coarse_rtol=1e-6)
            for what, wrong in stand_ins.items():
                worst, name = _rejected(lv, steps, wrong, vectors)
                print(f"{MC.KIND_NAME[kind]} {nx}x{ny}x{nz} block {which} steps {steps}: {what}: {worst:.2e} ({name})")
                assert worst > MC.CYCLE_BOUND, what
            # ... and accept what is right up to rounding: the same cycle with a direct coarsest solve, a permuted numbering
            pl, perm = MC.permuted(lv, 23)
            for what, right in [("direct coarsest solve", lambda r: MC.apply_reference(lv, r, steps, coarse_direct=True)),
                                ("permuted numbering", lambda r: MC.apply_permuted(pl, perm, r, steps))]:
                worst, name = _rejected(lv, steps, right, vectors)
                print(f"{MC.KIND_NAME[kind]} {nx}x{ny}x{nz} block {which} steps {steps}: drift under a {what}: {worst:.2e} ({name})")
                assert 100 * worst <= MC.CYCLE_BOUND


def test_loose_coarsest_solve_is_a_stand_in_on_most_kinds():
    tried = {m[0] for m in REJECT_MESHES if int((~_hier(*m, 0)[0][-1].mask).sum()) >= 20}
    assert len(tried) >= 3, tried


def test_fused_against_general_comparison_rejects_wrong_cycles():
    """The 1e-12 comparison of the two device cycles sees what the 1e-10 one sees."""
    lv, dims, _ = _hier(MC.HEX, 16, 16, 16, 0)
    vectors = MC.probe_vectors(lv, 17)
    wl = MC.with_transfer_weight(lv, dims, 2, 1e-6)
    worst, _ = _rejected(lv, 1, lambda r: MC.apply_reference(wl, r, 1), vectors)
    assert worst > MC.FUSED_BOUND


def test_fp32_discrepancy_is_far_from_the_fp64_bound():
    """Option mg_fp32: the NumPy cycle with fp32-rounded level operators in the smoother against the fp64 one (the GPU test
    takes 100 x this figure as its bound and asserts that the device's fp32 result is NOT the fp64 one)."""
    for kind, nx, ny, nz in [(MC.HEX, 12, 8, 16), (MC.TRI, 32, 32, 0)]:
        for which in (0, 1):
            lv, _, _ = _hier(kind, nx, ny, nz, which)
            A32 = MC.fp32_operators(lv)
            for steps in (1, 2):
                d = max(MC.rel_err(MC.apply_reference(lv, r, steps, smooth_A=A32), MC.apply_reference(lv, r, steps))
                        for _, r in MC.probe_vectors(lv, 29))
                print(f"{MC.KIND_NAME[kind]} {nx}x{ny}x{nz} block {which} steps {steps}: fp32 operators against fp64 {d:.2e}")
                assert 1e-9 < d < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# part 2: k iterations of PCG
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nx,ny,nz", [(MC.HEX, 16, 16, 16), (MC.QUAD, 40, 36, 0), (MC.TRI, 32, 32, 0), (MC.TET, 8, 8, 8)])
def test_sweep_comparison_rejects_a_wrong_first_dot_product(kind, nx, ny, nz):
    p = MC.sweep_problem(kind, nx, ny, nz)
    for k in (1, 2, 3):
        ref = MC.sweep_reference(p, k)
        bound = MC.sweep_bound(p, k)
        err = MC.rel_err(MC.sweep_reference(p, k, 1.0 + 1e-9), ref)
        wrong_cycle = MC.rel_err(MC.picard_sweep(p["A11"], p["A22"], p["A21"], p["rhs"],
                                                 lambda v: MC.apply_reference(p["levels"][0], v, 1, lam_from_next=1),
                                                 lambda v: MC.apply_reference(p["levels"][1], v, 1), k), ref)
        print(f"{MC.KIND_NAME[kind]} {nx}x{ny}x{nz} k {k}: bound {bound:.2e} (drift {MC.sweep_drift(p, k):.2e}), r.z x (1 + 1e-9): {err:.2e}, "
              f"level 2's smoother weight on level 1: {wrong_cycle:.2e}")
        assert err > bound and wrong_cycle > bound
        assert bound <= MC.CYCLE_BOUND
