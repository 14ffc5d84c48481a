"""Pins tests/post_reference.py, the reference of test_post_scale_gpu.py, on the CPU: against the oracle on small meshes of
all four kinds (ragged ones, 1 and 2 cells per direction), its restated launch rules against the cases of the GPU file,
and every comparison the GPU file makes against results that are wrong in one of the ways a kernel past its launch cap
can be wrong.  The reference's own bound is checked for attainability: the fp64 sums with the cells visited in a permuted
order stay inside max(100 delta, 1e-13)."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import post_reference as PR  # noqa: E402

from oracle import dpp_oracle as o  # noqa: E402

SMALL = [(PR.QUAD, 13, 7, 0), (PR.QUAD, 1, 1, 0), (PR.QUAD, 2, 2, 0), (PR.QUAD, 31, 17, 0),
         (PR.TRI, 9, 14, 0), (PR.TRI, 1, 1, 0), (PR.TRI, 2, 2, 0),
         (PR.HEX, 5, 4, 6), (PR.HEX, 1, 1, 1), (PR.HEX, 2, 2, 2), (PR.HEX, 7, 5, 6),
         (PR.TET, 4, 6, 3), (PR.TET, 1, 1, 1), (PR.TET, 2, 2, 2), (PR.TET, 5, 6, 3)]
RAGGED = [(PR.QUAD, 13, 7, 0), (PR.TRI, 9, 14, 0), (PR.HEX, 5, 4, 6), (PR.TET, 4, 6, 3)]
_ids = lambda c: f"{PR.KIND_NAME[c[0]]}{c[1]}x{c[2]}" + (f"x{c[3]}" if c[3] else "")  # noqa: E731


def _mesh(kind, nx, ny, nz):
    return o.build_mesh(PR.dim_of(kind), kind, nx, ny, nz)


@pytest.mark.parametrize("case", SMALL, ids=_ids)
def test_chunked_error_sums_equal_the_oracle(case):
    """nq = 1, 3, 6, 8; blocks and cell ranges that do not divide the cell count; the oracle's order of the points is its
    own, so only the sums are compared - within the reference's bound max(100 delta, 1e-13)"""
    kind = case[0]
    om = _mesh(*case)
    nodal, fields, ex = PR.norm_fields(om.coords)
    nc = om.num_cells
    for nq in (1, 3, 6, 8):
        ref = PR.norm_reference(kind, om.cells, om.coords, nq)
        for k in range(4):
            f = int(fields[k])
            l2, h1 = o.error_norms(om, nodal[k], lambda X: ex(X)[0][f], lambda X: ex(X)[1][f], nq)
            assert PR.norms_excess(ref, k, l2 * l2, h1 * h1) <= 1.0, (nq, k)
        for block, chunk in ((7, nc), (1 << 20, nc // 7 + 1), (100, nc // 3 + 1)):
            tot = {"l2": 0.0, "h1": 0.0}
            for c0 in range(0, nc, chunk):
                r = PR.error_sums(kind, om.cells, om.coords, nodal, fields, nq, exact=ex, block=block,
                                  cell_range=(c0, min(c0 + chunk, nc)))
                tot = {s: tot[s] + r[s] for s in tot}
            for k in range(4):
                assert PR.norms_excess(ref, k, tot["l2"][k], tot["h1"][k]) <= 1.0, (nq, block, chunk, k)


@pytest.mark.parametrize("case", RAGGED, ids=_ids)
def test_samples_points_and_per_cell_sums_are_consistent(case):
    """the exact field as samples at the returned points, in the layout of pph_quadrature_points over a range with
    c0 > 0, gives the sums of the callable; the per-cell sums add up; the points lie in their cells"""
    kind = case[0]
    om = _mesh(*case)
    d = om.dim
    nodal, fields, ex = PR.norm_fields(om.coords)
    nc = om.num_cells
    rng = (3, nc - 2)
    for nq in (1, 3):
        pts = PR.quadrature_points(kind, om.cells, om.coords, nq, rng)
        assert pts.shape == ((rng[1] - rng[0]) * nq ** d, d)
        X = om.coords[om.cells[rng[0]:rng[1]]]
        lo, hi = np.repeat(X.min(axis=1), nq ** d, axis=0), np.repeat(X.max(axis=1), nq ** d, axis=0)
        assert np.all(pts >= lo) and np.all(pts <= hi)
        P, G = ex(pts)
        a = PR.error_sums(kind, om.cells, om.coords, nodal[:1], [0], nq, exact=ex, cell_range=rng, per_cell=True)
        b = PR.error_sums(kind, om.cells, om.coords, nodal[:1], [0], nq, samples=(P[0], G[0]), cell_range=rng, block=11)
        for s in ("l2", "h1"):
            assert abs(a[s][0] - b[s][0]) <= PR.FLOOR * a[s][0]
            assert abs(a["cell_" + s][0].sum() - a[s][0]) <= PR.FLOOR * a[s][0]


@pytest.mark.parametrize("case", SMALL, ids=_ids)
def test_darcy_reference_equals_the_oracle(case):
    """right-hand side and projection against o.darcy_velocity, the matrix-free M x and diagonal against the oracle's M,
    the Kronecker solve against splu on the oracle's M; the bounds are those of the GPU file"""
    kind, nx, ny, nz = case
    om = _mesh(*case)
    d, n = om.dim, om.num_nodes
    _, M = o.assemble_scalar(om)
    p = PR.darcy_pressures(om.coords)
    b = PR.darcy_rhs(kind, om.cells, om.coords, p, PR.CONDUCTIVITY)
    lu = spla.splu(M.tocsc())
    u = np.stack([[lu.solve(b[k, e]) for e in range(d)] for k in range(2)])
    uo = np.stack([o.darcy_velocity(om, p[k], PR.CONDUCTIVITY).T for k in range(2)])
    drift = PR.residual_drift(kind, om.cells, om.coords, p[0], PR.CONDUCTIVITY, uo[0])
    assert 100 * drift < PR.CG_RTOL
    for cand in (u, uo):
        exc, fig = PR.darcy_excess(kind, om.cells, om.coords, p, cand, drift, direct=uo)
        assert max(exc.values()) <= 1.0, (exc, fig)
    # M x and the diagonal
    x = np.random.default_rng(5).standard_normal((3, n))
    y, D = PR.mass_apply(kind, om.cells, om.coords, x)
    yl, Dl = PR.mass_apply(kind, om.cells, om.coords, x, longdouble=True)
    dy = float(np.max(np.abs(y - yl) / np.abs(yl).max()))
    ref = (M @ x.T).T
    assert np.abs(y - ref).max() <= max(100 * dy, PR.FLOOR) * np.abs(ref).max()
    assert np.abs(D - M.diagonal()).max() <= PR.FLOOR * D.max()
    assert np.abs(D - np.asarray(Dl, np.float64)).max() <= PR.FLOOR * D.max()
    # Wathen's lower bound, which the derived error factor rests on
    S = M.toarray() / np.sqrt(np.outer(D, D))
    assert np.linalg.eigvalsh(S).min() >= PR.LAMBDA_MIN[kind] * (1 - 1e-12)
    if kind in (PR.QUAD, PR.HEX):
        uk = PR.kron_mass_solve((nx, ny, nz)[:d], b.reshape(2 * d, n)).reshape(2, d, n)
        exc, fig = PR.darcy_excess(kind, om.cells, om.coords, p, uk, drift, direct=u)
        assert max(exc.values()) <= 1.0, (exc, fig)


def test_restated_launch_rules_and_the_side_of_every_gpu_case():
    """pph_post.hip: norms_mms / norms_sampled / pph_quadrature_points launch min(ceil(cells / 256), 2048) workgroups of
    256, darcy() min(ceil(n / 256), 8192)"""
    assert PR.NORM_LANES == 2048 * 256 == 524288 and PR.DARCY_LANES == 8192 * 256 == 2097152
    assert PR.norm_launch(524288) == (2048, 1) and PR.norm_launch(524289) == (2048, 2) and PR.norm_launch(257) == (2, 1)
    assert PR.darcy_launch(2097152) == (8192, 1) and PR.darcy_launch(2097153) == (8192, 2)
    for name, (kind, nx, ny, nz) in PR.NORM_PAST.items():
        nc = PR.n_cells(kind, nx, ny, nz)
        assert PR.norm_launch(nc) == (2048, 2), name
        # the quadrature-point range of the GPU file: c0 > 0 and still more cells than lanes
        c0 = (nc - PR.NORM_LANES) // 2
        assert c0 > 0 and PR.norm_launch(nc - c0)[1] == 2, name
    assert PR.n_cells(*PR.NORM_PAST["quad1024x513"]) == 525312        # second pass: 1024 of 524 288 lanes busy
    assert PR.norm_launch(PR.n_cells(*PR.NORM_AT["quad1024x512"])) == (2048, 1)
    assert PR.n_cells(*PR.NORM_AT["quad1024x512"]) == PR.NORM_LANES
    for name, c in PR.NORM_SMALL.items():
        assert PR.norm_launch(PR.n_cells(*c))[1] == 1, name
    for name, c in PR.DARCY_PAST.items():
        assert PR.darcy_launch(PR.n_nodes(*c)) == (8192, 2), name
    assert PR.n_nodes(*PR.DARCY_PAST["quad1500x1400"]) == 2102901 and PR.n_nodes(*PR.DARCY_PAST["tet128x128x127"]) == 2130048
    for name, c in PR.DARCY_SMALL.items():
        assert PR.darcy_launch(PR.n_nodes(*c))[1] == 1, name
    assert PR.darcy_launch(PR.n_nodes(*PR.DARCY_SMALL["quad16x15"])) == (2, 1) and PR.n_nodes(*PR.DARCY_SMALL["quad16x15"]) == 272
    # every cell of a launch is added to exactly one slot; with the cap reached all 2048 are live
    nc = PR.n_cells(*PR.NORM_PAST["quad1024x513"])
    slots = PR.norm_slot(np.arange(nc), nc)
    assert slots.min() == 0 and slots.max() == 2047 and np.bincount(slots).min() == 256


# ----------------------------------------------------------------------------------------------------------------------
# the bound is attainable, and the comparisons see what they must
# ----------------------------------------------------------------------------------------------------------------------
# every mesh of the GPU file's norm cases
PERMUTED = [("small", n) for n in PR.NORM_SMALL] + [("past", n) for n in PR.NORM_PAST] + [("at", n) for n in PR.NORM_AT]
_REF = {}


def _norm_ref(kind, om, nq, name):
    """the reference of a mesh that more than one test uses is evaluated once (and left unchanged)"""
    if (name, nq) not in _REF:
        _REF[name, nq] = PR.norm_reference(kind, om.cells, om.coords, nq)
    return _REF[name, nq]


@pytest.mark.parametrize("where,name", PERMUTED)
def test_permuted_cell_order_stays_inside_the_bound(where, name):
    """the fp64 reference with its cells visited (and summed) in a random order is a second fp64 evaluation of the same
    sums: it must pass the comparison the device has to pass"""
    kind, nx, ny, nz = {"small": PR.NORM_SMALL, "past": PR.NORM_PAST, "at": PR.NORM_AT}[where][name]
    om = _mesh(kind, nx, ny, nz)
    for nq in ((1, 8) if where == "small" else (3,)):
        ref = _norm_ref(kind, om, nq, name)
        order = np.random.default_rng(3).permutation(om.num_cells)
        r = PR.error_sums(kind, om.cells, om.coords, ref["nodal"], ref["fields"], nq, exact=ref["exact"], order=order, block=5000)
        worst = max(PR.norms_excess(ref, k, r["l2"][k], r["h1"][k]) for k in range(4))
        print(f"{name} nq {nq}: delta L2 {ref['delta']['l2']}, delta H1 {ref['delta']['h1']}, permuted order at {worst:.2e} of the bound")
        assert worst <= 1.0


def test_norm_comparisons_reject_wrong_results():
    """quad 1024 x 513 (525 312 cells, nq 3): one 1D quadrature weight x (1 + 1e-6); the cells [524 288, ncell) skipped;
    partial-sum slot 2047 left out; the second chunk's samples read at the first chunk's offset - each must fail the
    comparison of every nodal field; and a quadrature-point array whose second pass was never written"""
    kind, nx, ny, nz = PR.NORM_PAST["quad1024x513"]
    om = _mesh(kind, nx, ny, nz)
    nq, nc = 3, om.num_cells
    ref = _norm_ref(kind, om, nq, "quad1024x513")
    nodal, fields, ex = ref["nodal"], ref["fields"], ref["exact"]
    pc = PR.error_sums(kind, om.cells, om.coords, nodal, fields, nq, exact=ex, per_cell=True)
    for k in range(4):
        assert PR.norms_excess(ref, k, pc["cell_l2"][k].sum(), pc["cell_h1"][k].sum()) <= 1.0
    x, w = PR.gauss_rule(nq)
    for i in (0, 1):                       # an end weight and the middle one
        w2 = w.copy()
        w2[i] *= 1.0 + 1e-6
        r = PR.error_sums(kind, om.cells, om.coords, nodal, fields, nq, exact=ex, rule=(x, w2))
        for k in range(4):
            assert PR.norms_excess(ref, k, r["l2"][k], r["h1"][k]) > 1.0, ("weight", i, k)
    keep = np.arange(nc) < PR.NORM_LANES
    live = PR.norm_slot(np.arange(nc), nc) != 2047
    for tag, mask in (("second pass skipped", keep), ("slot 2047 left out", live)):
        assert 0 < (~mask).sum() <= 1024
        for k in range(4):
            assert PR.norms_excess(ref, k, pc["cell_l2"][k][mask].sum(), pc["cell_h1"][k][mask].sum()) > 1.0, (tag, k)
    # sampled mode, chunks of 300 000 cells: the second chunk reads the first chunk's samples
    pts = PR.quadrature_points(kind, om.cells, om.coords, nq, (0, nc))
    P, G = ex(pts)
    chunk, npts = 300000, nq * nq
    for f in (0, 1):
        se, sg = P[f].copy(), G[f].copy()
        ks = [k for k in range(4) if fields[k] == f]
        good = PR.error_sums(kind, om.cells, om.coords, nodal[ks], [0] * len(ks), nq, samples=(se, sg))
        se[chunk * npts:], sg[chunk * npts:] = se[:(nc - chunk) * npts].copy(), sg[:(nc - chunk) * npts].copy()
        bad = PR.error_sums(kind, om.cells, om.coords, nodal[ks], [0] * len(ks), nq, samples=(se, sg))
        for i, k in enumerate(ks):
            assert PR.norms_excess(ref, k, good["l2"][i], good["h1"][i]) <= 1.0
            assert PR.norms_excess(ref, k, bad["l2"][i], bad["h1"][i]) > 1.0, ("sample offset", k)
    c0 = (nc - PR.NORM_LANES) // 2
    xref = PR.quadrature_points(kind, om.cells, om.coords, nq, (c0, nc))
    assert PR.points_excess(kind, xref * (1.0 + PR.U), xref) <= 1.0
    stale = xref.copy()
    stale[PR.NORM_LANES * npts:] = 0.0
    assert PR.points_excess(kind, stale, xref) > 1.0
    moved = xref.copy()
    moved[7, 1] += 1e-14
    assert PR.points_excess(kind, moved, xref) > 1.0


@pytest.mark.parametrize("name", ["quad61x47", "tri53x41", "hex37x5x11", "tet9x14x6"])
def test_darcy_comparisons_reject_wrong_results(name):
    """one incident cell dropped at one interior node of the right-hand side; two velocity components swapped; a solve
    stopped at 1e-9 instead of 1e-13"""
    kind, nx, ny, nz = PR.DARCY_SMALL[name]
    om = _mesh(kind, nx, ny, nz)
    d, n = om.dim, om.num_nodes
    _, M = o.assemble_scalar(om)
    lu = spla.splu(M.tocsc())
    p = PR.darcy_pressures(om.coords)
    b = PR.darcy_rhs(kind, om.cells, om.coords, p, PR.CONDUCTIVITY)
    u = np.stack([[lu.solve(b[k, e]) for e in range(d)] for k in range(2)])
    drift = PR.residual_drift(kind, om.cells, om.coords, p[0], PR.CONDUCTIVITY, u[0])
    direct = u if kind in (PR.QUAD, PR.HEX) else None
    exc, _ = PR.darcy_excess(kind, om.cells, om.coords, p, u, drift, direct=direct)
    assert max(exc.values()) <= 1.0
    inner = np.setdiff1d(np.arange(n), o.boundary_nodes(om))
    node = int(inner[len(inner) // 2])
    cell = int(np.nonzero((om.cells == node).any(axis=1))[0][0])
    one = PR.darcy_rhs(kind, om.cells[cell:cell + 1], om.coords, p, PR.CONDUCTIVITY)
    bad_b = b.copy()
    bad_b[:, :, node] -= one[:, :, node]
    dropped = np.stack([[lu.solve(bad_b[k, e]) for e in range(d)] for k in range(2)])
    swapped = u.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]
    early = u + 1e-9 * np.random.default_rng(2).standard_normal(u.shape) * np.abs(u).max()
    for tag, cand in (("dropped cell", dropped), ("swapped components", swapped), ("stopped early", early)):
        exc, fig = PR.darcy_excess(kind, om.cells, om.coords, p, cand, drift, direct=direct)
        assert exc["residual"] > 1.0, (tag, exc, fig)
        if direct is not None:
            assert exc["direct"] > 1.0, (tag, exc, fig)
        if tag != "stopped early":
            # (the linear pressure: every contribution of the dropped cell is the same constant, the swap exchanges
            # two different constants)
            assert exc["linear"] > 1.0, (tag, exc, fig)
