"""Self-checks of the vectorised degree-2 reference (tests/p2_matfree.py) against the cell-loop restatement
(tests/p2_restatement.py) and the CG-1 oracle, and the sensitivity of every comparison the GPU tests of
tests/test_p2_scale_gpu.py make: each must reject a reference-built stand-in for device output that is wrong by a
little."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import p2_matfree as F  # noqa: E402
import p2_restatement as R  # noqa: E402
import pmg_restatement as PM  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

K1, K2, BETA, MU = 1.0, 0.01, 1.0, 1.0
MESHES = {"quad5x3": (R.QUAD, 5, 3, 0), "quad7x4": (R.QUAD, 7, 4, 0), "tri5x3": (R.TRI, 5, 3, 0), "tri7x4": (R.TRI, 7, 4, 0),
          "hex3x4x2": (R.HEX, 3, 4, 2), "hex2x3x5": (R.HEX, 2, 3, 5), "tet3x4x2": (R.TET, 3, 4, 2), "tet2x3x5": (R.TET, 2, 3, 5)}


def _bc(kind, nx, ny, nz, variant):
    X = R.coords(kind, nx, ny, nz)
    b = R.boundary_nodes(kind, nx, ny, nz)
    if variant == 1:
        b = b[X[b, 0] < 1.0 - 1e-12]
    return b, np.exp(X[b, 0]) * np.sin(3 * X[b, 1]), np.cos(2 * X[b, 0]) + X[b, -1]


@pytest.mark.parametrize("name", list(MESHES))
def test_dofmap_and_pattern_closed_forms(name):
    kind, nx, ny, nz = MESHES[name]
    assert np.array_equal(F.dofmap_fast(kind, nx, ny, nz), R.dofmap(kind, nx, ny, nz))
    rowptr, col = R.pattern(kind, nx, ny, nz)
    lens = F.row_lengths(kind, nx, ny, nz)
    assert np.array_equal(lens, np.diff(rowptr))
    assert F.nnz_closed_form(kind, nx, ny, nz) == rowptr[-1]
    assert F.max_row(kind) >= lens.max()
    rp, cc = F.pattern_fast(kind, nx, ny, nz, chunk=5)
    assert np.array_equal(rp, rowptr) and np.array_equal(cc, col)
    if kind in (R.QUAD, R.HEX):
        # Q2: the length of a row is the product over the directions of 5 (even interior point) or 3 (any other)
        px, py, pz = R.lattice_dims(kind, nx, ny, nz)
        f = [np.where((np.arange(p) % 2 == 0) & (np.arange(p) > 0) & (np.arange(p) < p - 1), 5, 3) for p in (px, py, pz)]
        prod = (f[2][:, None, None] * f[1][None, :, None] * f[0][None, None, :]).ravel() if kind == R.HEX else \
            (f[1][:, None] * f[0][None, :]).ravel()
        assert np.array_equal(prod, np.diff(rowptr))


def test_max_rows_and_hex_nnz_limit():
    """The longest rows (the tile / LDS checks of pph_pmg use them) and the smallest Q2 hex past the int32 nnz limit."""
    assert {k: F.max_row(k) for k in (R.QUAD, R.TRI, R.HEX, R.TET)} == {
        k: int(np.diff(R.pattern(k, 4, 4, 4 if R.dim_of(k) == 3 else 0)[0]).max()) for k in (R.QUAD, R.TRI, R.HEX, R.TET)}
    assert F.max_row(R.HEX) == 125 and F.max_row(R.QUAD) == 25
    N = next(N for N in range(1, 400) if F.nnz_closed_form(R.HEX, N, N, N) >= 2 ** 31 - 1)
    assert (N, F.nnz_closed_form(R.HEX, N, N, N), F.nnz_closed_form(R.HEX, N - 1, N - 1, N - 1)) == \
        (162, 1297 ** 3, 1289 ** 3)


def _products(kind, nx, ny, nz, variant, seed=0, op=None):
    b, g1, g2 = _bc(kind, nx, ny, nz, variant)
    Kr, Mr = R.assemble_KM(kind, nx, ny, nz)
    A11, A22, A12, A21, rhs, u0 = R.eliminate(Kr, Mr, b, g1, g2, K1, K2, BETA, MU)
    n = Kr.shape[0]
    mask = np.zeros(n, bool)
    mask[b] = True
    rng = np.random.default_rng(seed)
    x1, x2 = rng.standard_normal(n), rng.standard_normal(n)
    loops = {"K": Kr @ x1, "M": Mr @ x1, "A11": A11 @ x1, "A22": A22 @ x2, "A12": A12 @ x2, "A21": A21 @ x1,
             "MONO": R.monolithic(A11, A22, A12, A21) @ np.concatenate([x1, x2])}
    fast = F.apply_blocks(kind, (nx, ny, nz), mask, x1, x2, K1, K2, BETA, MU, op=op)
    G1, G2 = np.zeros(n), np.zeros(n)
    G1[b], G2[b] = g1, g2
    lifted = F.lift(kind, (nx, ny, nz), mask, G1, G2, K1, K2, BETA, MU, op=op)
    return loops, fast, (rhs, u0), lifted


def _c(kind, w):
    return F.spmv_bound_factor(2 * F.max_row(kind) if w in ("MONO", "rhs") else F.max_row(kind), R.dim_of(kind))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", list(MESHES))
def test_matrix_free_products_equal_loop_restatement(name, variant):
    """Two evaluation orders of the reference (cell loop + SciPy CSR, vectorised bincount) stay within a tenth of the
    row-wise bound the GPU tests use."""
    kind, nx, ny, nz = MESHES[name]
    loops, fast, (rhs, u0), (r, mag, u) = _products(kind, nx, ny, nz, variant)
    for w, y in loops.items():
        e = F.row_excess(fast[w][0], y, fast[w][1], _c(kind, w))
        print(f"{name} variant {variant} {w}: {e:.3e}")
        assert e <= 0.1, w
    assert F.row_excess(r, rhs, mag, _c(kind, "rhs")) <= 0.1
    assert np.array_equal(u, u0)


@pytest.mark.parametrize("name", list(MESHES))
def test_norms_reference_equals_cg1_oracle(name):
    """On a CG-1 field (interpolated exactly into the degree-2 space) norms_reference is o.error_norms: same Gauss points,
    other summation order."""
    kind, nx, ny, nz = MESHES[name]
    d = R.dim_of(kind)
    om = o.build_mesh(d, kind, nx, ny, nz)
    ph1 = np.sin(2 * om.coords[:, 0]) + om.coords[:, 1] ** 2 - 0.5 * om.coords[:, -1]
    ph2 = PM.p_prolongation(kind, nx, ny, nz) @ ph1
    for field in (0, 1):
        p, g = F.mms_exact(field, d, K1, K2, BETA, MU)
        for nq in (3, 5):
            ref = F.norms_reference(kind, (nx, ny, nz), ph2, p, g, nq, chunk=7)
            l2, h1 = o.error_norms(om, ph1, p, g, nq=nq)
            assert ref["l2"] == pytest.approx(l2 ** 2, rel=1e-12, abs=0) and ref["h1"] == pytest.approx(h1 ** 2, rel=1e-12, abs=0)
    # the manufactured pressure restated here is the oracle's
    X = R.coords(kind, nx, ny, nz)
    par = o.Params(k1=K1, k2=K2, beta=BETA, mu=MU)
    for field in (0, 1):
        np.testing.assert_allclose(F.mms_exact(field, d, K1, K2, BETA, MU)[0](X), o.exact_pressures(X, par)[field],
                                   rtol=1e-15, atol=1e-15)


# ----------------------------------------------------------------------------------------------------------------------
# sensitivity: every comparison of the GPU tests rejects a stand-in that is wrong by a little
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quad7x4", "tri7x4", "hex2x3x5", "tet2x3x5"])
def test_products_reject_a_perturbed_element_entry_and_a_dropped_box(name):
    kind, nx, ny, nz = MESHES[name]
    op = F.Operator(kind, nx, ny, nz)
    _, good, _, _ = _products(kind, nx, ny, nz, 1, op=op)
    # one element-matrix entry x (1 + 1e-9): entry (a, b) of K_e of the last sub-cell type, a a free and b a constrained
    # node of the last cell (so that the lifted right-hand side sees it too), the largest such entry
    b_nodes = _bc(kind, nx, ny, nz, 1)[0]
    last = op.cells[-1, -1]
    Ke = op.elems[-1][0]
    a, b = max(((a, b) for a in range(op.m) for b in range(op.m)
                if last[a] not in b_nodes and last[b] in b_nodes), key=lambda ab: abs(Ke[ab]))
    elems = [(Ke_.copy(), Me_.copy()) for Ke_, Me_ in op.elems]
    elems[-1][0][a, b] *= 1.0 + 1e-9
    bad = F.Operator(kind, nx, ny, nz, elems=elems)
    _, wrong, _, (r_bad, _, _) = _products(kind, nx, ny, nz, 1, op=bad)
    _, _, _, (r, mag, _) = _products(kind, nx, ny, nz, 1, op=op)
    for w in ("K", "MONO"):
        assert F.row_excess(wrong[w][0], good[w][0], good[w][1], _c(kind, w)) > 1.0, w
    assert F.row_excess(r_bad, r, mag, _c(kind, "rhs")) > 1.0
    # the last box dropped: the dof map differs, the products of its rows too
    cut = F.Operator(kind, nx, ny, nz)
    cut.cells = cut.cells[:-1]
    assert not np.array_equal(cut.cells.reshape(-1, cut.m), F.dofmap_fast(kind, nx, ny, nz))
    _, dropped, _, (r_cut, _, _) = _products(kind, nx, ny, nz, 1, op=cut)
    for w in ("K", "M", "MONO"):
        assert F.row_excess(dropped[w][0], good[w][0], good[w][1], _c(kind, w)) > 1.0, w
    assert F.row_excess(r_cut, r, mag, _c(kind, "rhs")) > 1.0


@pytest.mark.parametrize("name", ["quad7x4", "hex2x3x5"])
def test_cycle_comparison_rejects_a_stale_tile(name):
    """The rows of one 32-row tile replaced by those of the previous tile (what a stale LDS tile would give)."""
    kind, nx, ny, nz = MESHES[name]
    b, _, _ = _bc(kind, nx, ny, nz, 0)
    n = R.n_nodes(kind, nx, ny, nz)
    mask = np.zeros(n, bool)
    mask[b] = True
    lv = PM.build_levels(kind, nx, ny, nz, K1 / MU, BETA / MU, mask)
    r = np.random.default_rng(3).standard_normal(n)
    r[mask] = 0.0
    ref = PM.cycle(lv, r, 2)
    t = (n // 32) // 2
    assert t >= 1
    stale = ref.copy()
    stale[32 * t:32 * (t + 1)] = ref[32 * (t - 1):32 * t]
    assert F.rel_max_error(stale, ref) > 1e-10
    assert F.rel_max_error(ref, ref) == 0.0


@pytest.mark.parametrize("name", ["quad7x4", "tri7x4", "hex2x3x5", "tet2x3x5"])
def test_norms_comparison_rejects_a_wrong_weight_and_a_skipped_range(name):
    kind, nx, ny, nz = MESHES[name]
    d = R.dim_of(kind)
    nq = 4
    X = R.coords(kind, nx, ny, nz)
    p, g = F.mms_exact(0, d, K1, K2, BETA, MU)
    pv = p(X)
    nodal = pv + 0.1 * np.abs(pv).max() * np.random.default_rng(31).uniform(-1.0, 1.0, pv.size)
    ref = F.norms_reference(kind, (nx, ny, nz), nodal, p, g, nq)
    ncell = F.dofmap_fast(kind, nx, ny, nz).shape[0]
    bound = F.norms_bound(ref, kind, ncell, nq)[:2]
    # another chunking of the same sums passes well inside the bound
    again = F.norms_reference(kind, (nx, ny, nz), nodal, p, g, nq, chunk=3)
    assert F.norms_excess((again["l2"], again["h1"]), ref, bound) <= 0.1
    # one quadrature weight x (1 + 1e-6)
    pts, wts = F.norm_rule(kind, nq)
    w2 = wts.copy()
    w2[len(w2) // 2] *= 1.0 + 1e-6
    bad = F.norms_reference(kind, (nx, ny, nz), nodal, p, g, nq, rule=(pts, w2))
    assert F.norms_excess((bad["l2"], bad["h1"]), ref, bound) > 1.0
    # a cell range skipped
    a = F.norms_reference(kind, (nx, ny, nz), nodal, p, g, nq, cell_range=(0, ncell // 2))
    z = F.norms_reference(kind, (nx, ny, nz), nodal, p, g, nq, cell_range=(ncell // 2 + 3, ncell))
    assert F.norms_excess((a["l2"] + z["l2"], a["h1"] + z["h1"]), ref, bound) > 1.0
    # the tensor weights of the rule are those of the kernel (0.5 per direction): a dropped factor is a factor 2
    assert np.sum(wts) == pytest.approx(1.0 if kind in (R.QUAD, R.HEX) else (0.5 if d == 2 else 1.0 / 6.0), rel=1e-14)


def test_ilu0_in_longdouble_matches_the_restatement():
    """p2_matfree.ilu0 in fp64 is R.ilu0; in longdouble it differs by a few units of the fp64 rounding."""
    kind, nx, ny, nz = MESHES["quad5x3"]
    b, g1, g2 = _bc(kind, nx, ny, nz, 0)
    Kr, Mr = R.assemble_KM(kind, nx, ny, nz)
    A11 = R.eliminate(Kr, Mr, b, g1, g2, K1, K2, BETA, MU)[0]
    r = np.random.default_rng(5).standard_normal(A11.shape[0])
    ref = R.ilu_apply(R.ilu0(A11), r)
    assert np.array_equal(F.ilu0(A11)[2], R.ilu0(A11)[2])
    ld = F.ilu_apply(F.ilu0(A11, np.longdouble), r.astype(np.longdouble))
    delta = float(np.max(np.abs(ref - ld)) / np.max(np.abs(ld)))
    assert 0.0 <= delta < 1e-13
