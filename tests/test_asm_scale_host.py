"""Host checks of tests/asm_scale_reference.py, the reference behind tests/test_asm_scale_gpu.py: the product against the
oracle's matrices and two other restatements, the eliminated blocks / right-hand sides against transient_reference, the restated
launch rules at their thresholds, the side of each threshold every GPU case is on, attainability of the GPU file's bounds by the
reference itself (fp64 against longdouble), and stand-ins for wrong kernels that every comparison of the GPU file must reject.

Tolerances of the small-mesh comparisons.  Two evaluations of one row in different orders differ by the rounding of their sums:
at most 64 products per row and piece (8 boxes x 8 corners), i.e. gamma_64 of the row magnitude in the worst case and a few eps
in practice: RESTATED = 32 eps (|A| |x|)_i.  The oracle integrates K and M on stored coordinates i / n, which carry an error of
n eps relative when n is no power of two (tests/test_transient_gpu.py::test_more_nodes_than_one_pass_of_the_grid): ORACLE = 64 eps.
Measured: the printouts, and tests/README_asm_scale.md."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import asm_scale_reference as R  # noqa: E402
import mg_cycle_reference as MC  # noqa: E402
import transient_reference as T  # noqa: E402
from oracle import dpp_mg_oracle as G  # noqa: E402

EPS = R.EPS
RESTATED, ORACLE = 32 * EPS, 64 * EPS
CF = R.CF
SIGMA = (7.5, 120.0)
NAMES = R.NAMES


def _id(c):
    return NAMES[c[0]] + "x".join(str(q) for q in c[1])


def _args(nd):
    return (nd[0], nd[1], nd[2] if len(nd) == 3 else 0)


def _sets(kind, nd, which):
    n = R.num_nodes(nd)
    i, j, k = R.node_ijk(nd)
    bnd = (i == 0) | (i == nd[0]) | (j == 0) | (j == nd[1])
    if len(nd) == 3:
        bnd |= (k == 0) | (k == nd[2])
    b = np.nonzero(bnd)[0]
    if which == "shared":
        return b, b
    m1 = (i == 0) | (j == nd[1])
    m1[n // 2] = True
    return b, np.nonzero(m1)[0]


@pytest.mark.parametrize("case", R.SMALL, ids=_id)
def test_box_apply_against_the_oracle_and_two_restatements(case):
    kind, nd = case
    om, K, M = T.scalar_matrices(len(nd), kind, *_args(nd))
    Kf, Mf = T.matfree_scalar_matrices(kind, *_args(nd))
    n = om.num_nodes
    assert n == R.num_nodes(nd)
    rng = np.random.default_rng(1)
    worst = [0.0, 0.0, 0.0]
    for cK, cM in ((1.0, 0.0), (0.0, 1.0), (1.3, 7.0), (0.01, 246.0)):
        for x in (rng.standard_normal(n), rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n), np.ones(n)):
            y, ab = R.box_apply(kind, nd, cK, cM, x), R.box_apply(kind, nd, cK, cM, x, absolute=True)
            assert np.all(ab >= abs(y) * (1 - 4 * EPS))
            refs = [cK * (K @ x) + cM * (M @ x), cK * (Kf @ x) + cM * (Mf @ x)]
            if kind in (R.QUAD, R.HEX):
                refs.append(MC.MatfreeOperator(_args(nd), cK, cM, np.zeros(n, bool)) @ x)
            for q, ref in enumerate(refs):
                worst[q] = max(worst[q], R.worst_fraction(y, ref, ab) / EPS)
            # the box-level magnitude is at least the entry-wise one (shares of one entry from several boxes, or from K and M, may cancel)
            assert np.all(ab * (1 + RESTATED) >= abs(cK * Kf + cM * Mf) @ abs(x))
    print(f"{_id(case)}: box_apply against the oracle {worst[0]:.2f} eps, matfree_scalar_matrices {worst[1]:.2f} eps, MatfreeOperator {worst[2]:.2f} eps "
          f"of (|A||x|)_i (bars {ORACLE / EPS:.0f}, {RESTATED / EPS:.0f}, {RESTATED / EPS:.0f})")
    assert worst[0] <= ORACLE / EPS and worst[1] <= RESTATED / EPS and worst[2] <= RESTATED / EPS


@pytest.mark.parametrize("case", R.SMALL, ids=_id)
def test_longdouble_product_and_both_diagonals(case):
    kind, nd = case
    n = R.num_nodes(nd)
    x = np.random.default_rng(2).standard_normal(n)
    y, yl = R.box_apply(kind, nd, 1.3, 7.0, x), R.box_apply(kind, nd, 1.3, 7.0, x, dtype=np.longdouble)
    assert yl.dtype == np.longdouble
    assert R.worst_fraction(y, yl.astype(np.float64), R.box_apply(kind, nd, 1.3, 7.0, x, absolute=True)) <= 8 * EPS
    Kf, Mf = T.matfree_scalar_matrices(kind, *_args(nd))
    for ab in (False, True):
        d, dc = R.diagonal(kind, nd, 1.3, 7.0, ab), R.diagonal_by_colouring(kind, nd, 1.3, 7.0, ab)
        assert abs(d - dc).max() <= 8 * EPS * abs(d).max()
        assert abs(d - (1.3 * Kf + 7.0 * Mf).diagonal()).max() <= 8 * EPS * abs(d).max()   # (diagonals: no cancellation, |.| changes nothing)


@pytest.mark.parametrize("sets", ["shared", "mixed"])
@pytest.mark.parametrize("case", R.SMALL, ids=_id)
def test_system_products_against_transient_reference(case, sets):
    """Eliminated blocks as products, the shifted right-hand side and step_rhs against shifted_blocks / step_rhs."""
    kind, nd = case
    Kf, Mf = T.matfree_scalar_matrices(kind, *_args(nd))
    n = Kf.shape[0]
    nodes = _sets(kind, nd, sets)
    masks = T.masks_of(n, *nodes)
    g = R.dirichlet_data(n, nodes)
    rng = np.random.default_rng(3)
    worst = 0.0
    for sigma in (SIGMA, (0.0, 31.0), (0.0, 0.0)):
        S = R.System(kind, nd, CF, sigma, masks, g)
        A11, A22, A12, A21, rhs, u0 = T.shifted_blocks(Kf, Mf, CF, sigma, masks, g)
        mats = dict(zip(R.WHICH, (A11, A22, A12, A21, sp.bmat([[A11, A12], [A21, A22]], format="csr"))))
        for w in R.WHICH:
            x = rng.standard_normal(2 * n if w == "MONO" else n)
            worst = max(worst, R.worst_fraction(S.apply(w, x), mats[w] @ x, S.apply(w, x, True)))
            assert np.all(S.apply(w, x, True) * (1 + RESTATED) >= abs(mats[w]) @ abs(x))
        worst = max(worst, R.worst_fraction(S.rhs(), rhs, S.rhs(True)))
        assert np.array_equal(S.u0(), u0)
        for f, A in ((0, A11), (1, A22)):
            assert abs(S.diag(f) - A.diagonal()).max() <= 8 * EPS * A.diagonal().max()
        p = rng.standard_normal(2 * n)
        worst = max(worst, R.worst_fraction(S.step_rhs(p), T.step_rhs(Kf, Mf, CF, masks, p), S.step_rhs(p, True)))
        assert np.all(S.step_rhs(p, True) * (1 + RESTATED) >= np.where(np.concatenate(masks), 0.0, T.abs_bound(Kf, Mf, CF, p)))
        # longdouble runs through box_apply itself, fp64 through the shared pieces: a few eps apart
        Sl = R.System(kind, nd, CF, sigma, masks, g, np.longdouble)
        x = rng.standard_normal(2 * n)
        assert R.worst_fraction(S.apply("MONO", x), Sl.apply("MONO", x).astype(np.float64), S.apply("MONO", x, True)) <= 8 * EPS
    print(f"{_id(case)} {sets}: worst {worst / EPS:.2f} eps of the row magnitude (bar {RESTATED / EPS:.0f})")
    assert worst <= RESTATED


# -- launch rules -------------------------------------------------------------------------------------------------------------
def test_launch_rules_at_their_thresholds():
    # tiles: 64 x 64 = 4096 tiles of 16 x 8 nodes in one pass; 17 x 241 = 4097 in two
    L = R.tile_launch(R.QUAD, (1023, 511))
    assert (L["ntiles"], L["grid"], L["passes"]) == (4096, 4096, 1)
    L = R.tile_launch(R.QUAD, (256, 1920))
    assert (L["ntiles"], L["grid"], L["passes"]) == (4097, 4096, 2)
    t = R.tile_pass(np.arange(4097), L)
    assert t[4095] == 0 and t[4096] == 1
    L = R.tile_launch(R.HEX, (127, 63, 15))       # 16 x 16 x 8 = 2048 tiles ... and 16 x 16 x 16 = 4096, 16 x 16 x 17
    assert L["ntiles"] == 2048 and L["passes"] == 1
    assert R.tile_launch(R.HEX, (127, 63, 31))["passes"] == 1 and R.tile_launch(R.HEX, (127, 63, 32))["passes"] == 2
    # xmap: from 64 workgroups on; a multiple of 8 workgroups; every XCD strides through its own eighth
    assert R.tile_launch(R.QUAD, (100, 30), 1)["xmap"] == 0 and R.tile_launch(R.QUAD, (127, 63), 1)["xmap"] == 1
    L = R.tile_launch(R.QUAD, (1024, 512), 1)
    assert (L["ntiles"], L["grid"], L["tpx"], L["step"], L["passes"]) == (4225, 4096, 529, 512, 2)
    L = R.tile_launch(R.HEX, (40, 20, 10), 1)     # 6 x 6 x 6 = 216 tiles: grid 216, a multiple of 8 already; 27 per XCD, one pass
    assert (L["grid"], L["tpx"], L["step"], L["passes"]) == (216, 27, 27, 1)
    L = R.tile_launch(R.QUAD, (16 * 7 - 1, 8 * 11 - 1), 1)   # 77 tiles: 72 workgroups, 10 tiles per XCD on 9 workgroups: two passes
    assert (L["ntiles"], L["grid"], L["tpx"], L["step"], L["passes"]) == (77, 72, 10, 9, 2)
    # every tile is visited exactly once, xmap or not (the kernel's loop: t_first, t_step, t_end)
    for xm in (0, 1):
        L = R.tile_launch(R.QUAD, (16 * 7 - 1, 8 * 11 - 1), xm)
        seen = []
        for wg in range(L["grid"]):
            if L["xmap"]:
                xcd, bxx = wg & 7, wg >> 3
                first, end = xcd * L["tpx"] + bxx, min((xcd + 1) * L["tpx"], L["ntiles"])
            else:
                first, end = wg, L["ntiles"]
            tiles = list(range(first, end, L["step"]))
            seen += tiles
            assert [int(q) for q in R.tile_pass(np.array(tiles, dtype=np.int64), L)] == list(range(len(tiles)))
        assert sorted(seen) == list(range(L["ntiles"]))
    # thread-per-item kernels
    for cap, fn in ((R.STEP_MAX_WG, R.step_rhs_launch), (R.SIMPLEX_MAX_WG, R.simplex_launch), (R.NODE_MAX_WG, R.node_launch)):
        assert fn(cap * 256)["passes"] == 1 and fn(cap * 256)["grid"] == cap
        assert fn(cap * 256 + 1)["passes"] == 2 and fn(cap * 256 + 1)["grid"] == cap
    assert R.step_rhs_launch(2048 * 256) == {"grid": 2048, "stride": 524288, "passes": 1}
    assert T.step_kernel_loops(2048 * 256 + 1) and not T.step_kernel_loops(2048 * 256)
    assert R.step_update_launch(262144)["passes"] == 1 and R.step_update_launch(262145)["passes"] == 2
    assert R.step_update_launch(262143)["grid"] == 2048 and R.step_update_launch(261000)["grid"] < 2048
    assert R.mono_launch(4096 * 256 - 1)["rowptr_passes"] == 1 and R.mono_launch(4096 * 256)["rowptr_passes"] == 2
    assert R.mono_launch(4096 * 32)["fill_passes"] == 1 and R.mono_launch(4096 * 32 + 1)["fill_passes"] == 2
    assert R.node_launch(1000)["grid"] == 8 and R.node_launch(199999)["split"] == 0 and R.node_launch(200000)["split"] == 1
    # two-pass kernels: 4096 batches of 32 hex / 64 quad nodes or cells
    L = R.two_pass_launch(R.HEX, (31, 31, 127))
    assert (L["per"], L["cell_batches"] <= 4096, L["node_batches"], L["node_passes"]) == (32, True, 4096, 1)
    assert R.two_pass_launch(R.QUAD, (511, 511))["node_passes"] == 1 and R.two_pass_launch(R.QUAD, (512, 511))["node_passes"] == 2
    # the family
    assert R.assembly_path(R.TRI, 10, True) == R.assembly_path(R.TET, 10 ** 7, False) == "simplex"
    assert R.assembly_path(R.HEX, 100, True) == "node" and R.assembly_path(R.HEX, 100, True, ell=False) == "two-pass"
    assert R.assembly_path(R.HEX, 29999, False) == "two-pass" and R.assembly_path(R.HEX, 30000, False) == "tile"
    assert R.assembly_path(R.QUAD, 100, False, asm_tile=2) == "tile" and R.assembly_path(R.QUAD, 10 ** 6, False, asm_tile=0) == "two-pass"
    assert R.assembly_path(R.QUAD, 10 ** 6, True, asm_node=0) == "tile" and R.assembly_path(R.QUAD, 1 << 29, True) == "tile"


def test_every_gpu_case_is_past_its_threshold():
    """What tests/test_asm_scale_gpu.py asserts on the GPU, here without one."""
    want = {"hex128x64x64": (545025, 9537, 3, 3, 17033, 5, 2), "quad1024x512": (525825, 4225, 2, 2, 8217, 3, 2)}
    for name, (n, ntiles, passes, xpasses, batches, bpasses, spasses) in want.items():
        kind, nd = R.CASES[name]
        assert R.num_nodes(nd) == n and R.assembly_path(kind, n, False) == "tile" and R.assembly_path(kind, n, True) == "node"
        L, X, B = R.tile_launch(kind, nd), R.tile_launch(kind, nd, 1), R.two_pass_launch(kind, nd)
        assert (L["ntiles"], L["passes"], X["passes"], B["node_batches"], B["node_passes"]) == (ntiles, passes, xpasses, batches, bpasses)
        assert B["cell_passes"] >= 2 and R.step_rhs_launch(n)["passes"] == spasses and R.step_update_launch(n)["passes"] >= 2
    assert MC.level_nodes(R.HEX, 128, 64, 64)[:3] == [545025, 70785, 9537]
    assert R.assembly_path(R.HEX, 70785, False) == "tile" and R.assembly_path(R.HEX, 9537, False) == "two-pass"
    for name, n, passes, spasses in (("tri2048x1024", 2100225, 2, 5), ("tet128", 2146689, 2, 5)):
        kind, nd = R.CASES[name]
        assert R.num_nodes(nd) == n and R.assembly_path(kind, n, False) == "simplex"
        assert R.simplex_launch(n)["passes"] == passes and R.step_rhs_launch(n)["passes"] == spasses
    for name, n in (("quad2048", 4198401), ("hex256x128x128", 4276737)):
        kind, nd = R.CASES[name]
        L = R.node_launch(n)
        assert R.num_nodes(nd) == n and R.assembly_path(kind, n, True) == "node" and (L["grid"], L["passes"], L["split"]) == (16384, 2, 1)
        assert n > 64 * L["windows_per_launch"]
        Lm = R.mono_launch(n)       # the monolithic matrix of these cases: k_mono_rowptr and k_mono_fill loop
        assert (Lm["rowptr_grid"], Lm["fill_grid"]) == (4096, 4096) and Lm["rowptr_passes"] == 5 and Lm["fill_passes"] == 33
    # a constrained interior node of field 1 in the last pass of every launch in question; odd node counts
    for name, (kind, nd) in R.CASES.items():
        n = R.num_nodes(nd)
        assert n % 2 == 1 and all(q & (q - 1) == 0 for q in nd)
        nodes = R.dirichlet_sets(kind, nd)
        m0, m1 = T.masks_of(n, *nodes)
        inner1 = m1 & ~m0
        assert R.INTERIOR_PICKS <= np.count_nonzero(inner1) <= R.INTERIOR_PICKS + 1
        paths = [("step", 0)]
        if name in R.UNSHIFTED_ONLY:
            paths.append(("node", 0))
        elif kind in (R.TRI, R.TET):
            paths.append(("simplex", 0))
        else:
            paths += [("tile", 0), ("tile", 1), ("two-pass", 0)]
        for path, xm in paths:
            last = R.last_pass_rows(kind, nd, path, xm)
            assert 0 < np.count_nonzero(last) < n and np.count_nonzero(inner1 & last) >= 1, (name, path, xm)


# -- attainability and stand-ins --------------------------------------------------------------------------------------------------
_cases = {}


def _case(name):
    if name not in _cases:
        _cases.clear()
        R.clear_pieces()
        kind, nd = R.CASES[name]
        n = R.num_nodes(nd)
        nodes = R.dirichlet_sets(kind, nd)
        masks = T.masks_of(n, *nodes)
        _cases[name] = (kind, nd, n, masks, R.dirichlet_data(n, nodes))
    return _cases[name]


@pytest.mark.parametrize("name", list(R.SHIFTED))
def test_the_reference_attains_a_tenth_of_the_bound(name):
    """fp64 against longdouble, on the meshes of the GPU file themselves: the monolithic product of a normal vector (all four
    blocks), the lifted right-hand side and step_rhs stay below BAR / 10 of the row magnitude."""
    kind, nd, n, masks, g = _case(name)
    sigma = R.dominant_sigma(CF, nd[0])
    S, Sl = R.System(kind, nd, CF, sigma, masks, g), R.System(kind, nd, CF, sigma, masks, g, np.longdouble)
    x = np.random.default_rng(7).standard_normal(2 * n)
    fr = [R.worst_fraction(S.apply("MONO", x), Sl.apply("MONO", x).astype(np.float64), R.BAR * S.apply("MONO", x, True)),
          R.worst_fraction(S.rhs(), Sl.rhs().astype(np.float64), R.BAR * S.rhs(True))]
    if name == "hex128x64x64":
        fr.append(R.worst_fraction(S.step_rhs(x), Sl.step_rhs(x).astype(np.float64), R.BAR * S.step_rhs(x, True)))
    print(f"{name}: the fp64 reference against longdouble: {', '.join(f'{q:.1e}' for q in fr)} of the bound ({max(fr) * 1e3:.2f} eps of the row magnitude)")
    assert max(fr) <= 0.1


def test_rows_whose_bound_rests_on_a_cancelling_stiffness_entry():
    """The rows where BAR (|A| |x|)_i holds only for an evaluation whose directional stiffness terms cancel EXACTLY, found by
    test_asm_scale_gpu.py (hex 128x64x64, asm_tile_xmap 1, sigma (0, 31), block A11, the vector that lives on the last pass: 1.10 of
    the bound before k_asm_tile's reference-element table was put in closed form, 0.006 after).  On 128 x 64 x 64 cells the three
    directional terms of KB cancel exactly for the corner pairs that differ in y and z, so the bound holds only the mass share of
    those entries, while an evaluation that sums rounded terms leaves a rounding of the size of the TERMS.  A row whose only
    non-zero neighbours are such entries - the vector is sparse, and Dirichlet columns are eliminated - has a bound 2000 times
    below the magnitude of what is added up.  The longdouble comparison above cannot see it (both sides read the same KB)."""
    kind, nd, n, masks, g = _case("hex128x64x64")
    KB, MB = T.box_matrices(kind, list(nd))
    KT = R.stiffness_term_magnitudes(kind, nd)
    assert np.count_nonzero(KB == 0.0) == 8 and np.all(KT[KB == 0.0] > 0.08 * abs(KB).max())
    assert np.all(KT >= abs(KB) * (1 - 4 * EPS)) and (KT / np.where(KB == 0.0, np.inf, abs(KB))).max() < 2.5
    a, b, _ = CF.abc
    F = (~masks[0]).astype(np.float64)
    worst = {}
    for xm in (0, 1):
        vL = R.probe_vectors(n, R.last_pass_rows(kind, nd, "tile", xm), 7)[2]
        X = abs(F * vL).reshape(R.shape_of(nd))
        bound = F * R.gather(a * abs(KB) + b * abs(MB), X).ravel()
        terms = F * R.gather(a * KT + b * abs(MB), X).ravel()
        assert np.allclose(bound, R.System(kind, nd, CF, (0.0, 31.0), masks, g).apply("A11", vL, True) * F, rtol=1e-13, atol=0)   # (the GPU file's bound)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(bound > 0, terms / bound, 0.0)
        worst[xm] = (float(q.max()), int(np.count_nonzero(q > 50)))
    print(f"hex 128x64x64, A11 with sigma1 = 0, last-pass vector: magnitude of the summed terms over the bound, worst row: {worst[0][0]:.0f} "
          f"(round-robin tiles), {worst[1][0]:.0f} (xmap; {worst[1][1]} rows above 50)")
    # one rounding of the terms (eps / 2 each) is BAR * bound / 1000 * ratio / 2: from a ratio of 2000 on the bar is used up
    assert worst[1][0] > 1900 and worst[0][0] < 100
    # the reference itself moves by more than the bound there when KB's cancelling entries are off by one ulp of their terms
    KB1 = KB + np.where(KB == 0.0, np.spacing(KT), 0.0)
    vL = R.probe_vectors(n, R.last_pass_rows(kind, nd, "tile", 1), 7)[2]
    X = (F * vL).reshape(R.shape_of(nd))
    y0, y1 = F * R.gather(a * KB + b * MB, X).ravel(), F * R.gather(a * KB1 + b * MB, X).ravel()
    bound = F * R.gather(a * abs(KB) + b * abs(MB), abs(X)).ravel()
    assert not R.within_bar(y1, y0, bound)


def _blank(y, rows):
    z = y.copy()
    z[rows] = 0.0
    return z


def test_stand_ins_for_wrong_assembly_kernels_are_rejected():
    """Each stand-in is the reference output with one defect a wrong kernel would leave, at the size of the smallest GPU case of
    its kind; the comparison of the GPU file (asm_scale_reference.within_bar, the vectors of probe_vectors) must reject it."""
    for name, paths in (("quad1024x512", (("tile", 0), ("tile", 1), ("two-pass", 0))), ("hex128x64x64", (("tile", 0), ("tile", 1), ("two-pass", 0))),
                        ("tri2048x1024", (("simplex", 0),))):
        kind, nd, n, masks, g = _case(name)
        sigma = R.dominant_sigma(CF, nd[0])
        S = R.System(kind, nd, CF, sigma, masks, g)
        for path, xm in paths:
            last = R.last_pass_rows(kind, nd, path, xm)
            v = R.probe_vectors(n, last, 7)
            ref = [S.apply("A22", x) for x in v]
            bound = [S.apply("A22", x, True) for x in v]
            assert all(R.within_bar(y, y, b) for y, b in zip(ref, bound))
            # the rows of the last pass (tile, batch, node per thread) left zero: every vector sees it, the third one ONLY there
            for y, b in zip(ref, bound):
                assert not R.within_bar(_blank(y, last), y, b), (name, path, xm)
            assert np.array_equal(_blank(ref[2], ~last)[last], ref[2][last])
        # one stored entry x (1 + 1e-9): the diagonal entry of a free row of the last pass
        row = int(np.nonzero(last & ~masks[1])[0][-1])
        d = S.diag(1)
        hit = 0
        for x, y, b in zip(v, ref, bound):
            z = y.copy()
            z[row] += 1e-9 * d[row] * x[row]
            hit += not R.within_bar(z, y, b)
        assert hit >= 2, name
        dz = d.copy()
        dz[row] *= 1 + 1e-9
        assert abs(1 / dz - 1 / d)[row] > R.BAR * (S.diag(1, True) / (d * d))[row]     # (the inverse-diagonal comparison sees it too)
        # the entry-wise export (VAL_TOL = 1e-12 of the LARGEST entry, the unit rows' 1) sees it in A11; A22's entries, smaller by
        # k2 / k1 against the same unit rows, are below that bar: there the products and the inverse diagonal are what sees it
        d0 = S.diag(0)
        row0 = int(np.nonzero(last & ~masks[0])[0][-1])
        assert 1e-9 * d0[row0] > 1e-12 * d0.max()
        # sigma1 and sigma2 exchanged: products, inverse diagonal, right-hand side
        X = R.System(kind, nd, CF, sigma[::-1], masks, g)
        assert not R.within_bar(X.apply("A22", v[0]), ref[0], bound[0]) and not R.within_bar(X.apply("A11", v[1]), S.apply("A11", v[1]), S.apply("A11", v[1], True))
        assert not R.within_bar(X.rhs(), S.rhs(), S.rhs(True))
        assert (abs(1 / X.diag(0) - 1 / S.diag(0)) / (R.BAR * S.diag(0, True) / S.diag(0) ** 2)).max() > 1.0
        # the lift share (sigma_f F_f M g_f, k_step_rhs<KIND, true>) missing on the rows from 524 288 on
        lift_last = np.arange(n) >= R.STEP_MAX_WG * R.BLOCK
        assert R.step_rhs_launch(n)["passes"] >= 2 and lift_last.any()
        plain = R.System(kind, nd, CF, (0.0, 0.0), masks, g).rhs()
        both = np.concatenate([lift_last, lift_last])
        z = np.where(both, plain, S.rhs())
        assert not R.within_bar(z, S.rhs(), S.rhs(True)), name
        assert R.within_bar(np.where(both, S.rhs(), S.rhs()), S.rhs(), S.rhs(True))


def test_stand_ins_for_wrong_levels_and_step_sums_are_rejected():
    kind, nd, n, masks, g = _case("hex128x64x64")
    sigma = R.dominant_sigma(CF, nd[0])
    a, b, c = CF.abc
    # a level operator built with the unshifted mass coefficient (level 1: the tile kernel as a level-operator producer; level 2:
    # the two-pass kernels)
    lv = MC.matfree_hierarchy(kind, nd[0], nd[1], nd[2], c, b + sigma[1], masks[1])
    plain = MC.matfree_hierarchy(kind, nd[0], nd[1], nd[2], c, b, masks[1])
    vectors = MC.probe_vectors(lv, 12)[:3]
    for l in (1, 2):
        bad = list(lv)
        bad[l] = G.Level(plain[l].A, plain[l].dinv, plain[l].mask, plain[l].lam)
        bad[l].P = lv[l].P
        worst = 0.0
        for ns in (1, 2):
            errs = [MC.rel_err(MC.apply_reference(bad, r, ns), MC.apply_reference(lv, r, ns)) for _, r in vectors]
            worst = max(worst, min(errs))
            assert max(errs) > 1e3 * MC.CYCLE_BOUND, (l, ns, errs)
        print(f"level {l} built without the shift: every probing vector off by at least {worst:.1e} (bound {MC.CYCLE_BOUND:.0e})")
    # partial-sum slot 2047 of k_step_update left out of ||d||^2: workgroup 2047 holds the entries (i // 256) % 2048 == 2047
    L = R.step_update_launch(n)
    assert L["grid"] == 2048
    d = np.random.default_rng(5).standard_normal(2 * n)
    d[np.concatenate(masks)] = 0.0
    slot = (np.arange(2 * n) // R.BLOCK) % L["grid"]
    rel, tol = R.norm_check(float(np.linalg.norm(d)), d)
    assert rel <= tol
    rel, tol = R.norm_check(float(np.sqrt(np.dot(d[slot != 2047], d[slot != 2047]))), d)
    assert rel > 1e6 * tol
    # ... and written one slot low (slot 0 lost, no other): the same size of error
    rel, tol = R.norm_check(float(np.sqrt(np.dot(d[slot != 0], d[slot != 0]))), d)
    assert rel > 1e6 * tol
    _cases.clear()
    R.clear_pieces()
