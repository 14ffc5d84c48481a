"""CG-1 assembly (perphil_amd/csrc/pph_assemble.hip) and the step kernels (pph_transient.hip) past their launch caps, against
the matrix-free fp64 reference of tests/asm_scale_reference.py.

A system with a storage shift (pph_assemble_dpp_shifted, sigma != 0) never takes the node kernel: it is assembled by
k_asm_tile from 30 000 nodes on, by k_elem_rows + k_gather_rows below, by k_asm_simplex_gather<., true> on simplices, and the
shift's share of the lifting is a launch of k_step_rhs<KIND, true>.  The meshes here put each of them past its grid cap
(asm_scale_reference.CASES and its restated launch rules; every case asserts which side of its threshold it is on):

  hex 128x64x64    545 025 nodes: 9537 tiles (up to 3 per workgroup), 17 033 node batches of the two-pass kernels, 2 passes of
                   the step kernels; multigrid levels of 70 785 (tile kernel) and 9537 nodes (two-pass kernels)
  quad 1024x512    525 825 nodes: 4225 tiles, 8217 node batches
  tri 2048x1024    2 100 225 nodes: a second node per thread of the simplex gather, 5 passes of the step kernel
  tet 128^3        2 146 689 nodes: the same in 3D
  quad 2048^2, hex 256x128x128 (unshifted): 4 198 401 / 4 276 737 nodes, past the node kernel's 16 384 x 256 rows

Cell counts are powers of two (the device integrates on stored coordinates i / n, exact only then); the node counts are odd, so
the last tile is partly filled in every direction.  Field 0 is constrained on the whole boundary, field 1 on two sides plus
interior nodes of which at least one lies in the last pass of the launch in question (asserted); values uniform in [0.5, 1.5].

Bounds.  Products, right-hand sides and step_rhs: |got_i - ref_i| <= BAR (|A| |x|)_i row by row, BAR = 1e3 eps, the project's
bar for the step right-hand side, (|A| |x|) from box_apply(absolute=True).  Inverse diagonals: the same BAR, relative.
Entry-wise exports: VAL_TOL = 1e-12 of the largest entry (tests/test_transient_gpu.py).  Level operators: 1e-10 max |ref|
(tests/test_mg_cycle_gpu.py).  Norms of the step loop: max(100 delta, 1e-13) relative, delta the fp64 sum against longdouble.
Residual of a step: ||D^-1 r|| <= (rtol + 100 drift) ||D^-1 b||, the solver's own stopping rule plus the reference's
evaluation drift.  No bound was chosen from the device's output; every case prints its worst fraction before it asserts.
Measured figures: tests/README_asm_scale.md."""
import os
import sys
import time

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from perphil_amd import _ffi  # noqa: E402
from perphil_amd import solver, solver_parameters as spar  # noqa: E402
import asm_scale_reference as R  # noqa: E402
import mg_cycle_reference as MC  # noqa: E402
import transient_reference as T  # noqa: E402

pytestmark = pytest.mark.gpu

CF = R.CF
BAR = R.BAR
VAL_TOL = 1e-12
MATS = {"A11": _ffi.MAT_A11, "A22": _ffi.MAT_A22, "A12": _ffi.MAT_A12, "A21": _ffi.MAT_A21, "MONO": _ffi.MAT_MONO}

OPTION_SETS = {
    # name: (options, shifted, path of the fine level by the restated rules, xmap)
    "shifted": ((), True, "tile", 0),
    "shifted-xmap": ((("asm_tile_xmap", 1),), True, "tile", 1),
    "shifted-two-pass": ((("asm_tile", 0),), True, "two-pass", 0),
    "shifted-csr": ((("op_format", 0),), True, "tile", 0),
    "unshifted-tile": ((("asm_node", 0),), False, "tile", 0),
}
SIMPLEX_SETS = {"shifted": ((), True, "simplex", 0), "unshifted": ((), False, "simplex", 0)}
RUNS = [(c, s) for c in ("hex128x64x64", "quad1024x512") for s in OPTION_SETS] + \
       [(c, s) for c in ("tri2048x1024", "tet128") for s in SIMPLEX_SETS]

_case_cache = {}


def _case(name):
    """Mesh, Dirichlet sets and data of a case; one case at a time is kept (with its shared reference products)."""
    if name not in _case_cache:
        _case_cache.clear()
        R.clear_pieces()
        kind, nd = R.CASES[name]
        n = R.num_nodes(nd)
        nodes = R.dirichlet_sets(kind, nd)
        _case_cache[name] = {"kind": kind, "nd": nd, "n": n, "nodes": nodes, "masks": T.masks_of(n, *nodes),
                             "g": R.dirichlet_data(n, nodes)}
    return _case_cache[name]


def _context(make, c, options=()):
    ctx = make()
    for name, v in options:
        ctx.set_option(name, v)
    nd = c["nd"]
    ctx.mesh_build(len(nd), c["kind"], nd[0], nd[1], nd[2] if len(nd) == 3 else 0)
    assert ctx.n == c["n"]
    for f in (0, 1):
        ctx.set_dirichlet(f, c["nodes"][f], c["g"][f][c["nodes"][f]])
    return ctx


def _describe(kind, nd, path, xmap):
    n = R.num_nodes(nd)
    if path == "tile":
        L = R.tile_launch(kind, nd, xmap)
        return f"k_asm_tile{' xmap' if L['xmap'] else ''}: {L['ntiles']} tiles on {L['grid']} workgroups, up to {L['passes']} per workgroup", L["passes"]
    if path == "two-pass":
        L = R.two_pass_launch(kind, nd)
        return (f"k_elem_rows + k_gather_rows: {L['cell_batches']} cell / {L['node_batches']} node batches, up to {L['cell_passes']} / "
                f"{L['node_passes']} per workgroup"), min(L["cell_passes"], L["node_passes"])
    if path == "simplex":
        L = R.simplex_launch(n)
        return f"k_asm_simplex_gather: {n} nodes on {L['grid']} x 256 threads, up to {L['passes']} per thread", L["passes"]
    L = R.node_launch(n)
    return f"k_asm_node2: {n} nodes on {L['grid']} x 256 threads, up to {L['passes']} per thread, split {L['split']}", L["passes"]


def _within(tag, got, ref, bound, worst):
    """Records the worst fraction of the bound; a comparison that misses it is kept in worst[2] and asserted by the caller at the
    end of the case, so that every comparison of a case runs and is reported."""
    frac = R.worst_fraction(got, ref, BAR * bound)
    worst[0] = max(worst[0], frac)
    if not frac <= 1.0:
        worst[2].append((tag, frac))


def _check_products(tag, ctx, S, vectors, worst, which=R.WHICH):
    n = S.n
    for w in which:
        for vi, x in enumerate(vectors):
            xx = np.concatenate([x, vectors[(vi + 1) % len(vectors)]]) if w == "MONO" else x
            _within(f"{tag} {w} vector {vi}", ctx.spmv(MATS[w], xx), S.apply(w, xx), S.apply(w, xx, True), worst)
    assert n == ctx.n


def _check_rhs_and_diagonal(tag, ctx, S, last, worst):
    r, u0 = ctx.rhs()
    ref, bound = S.rhs(), S.rhs(True)
    _within(f"{tag} rhs", r, ref, bound, worst)
    con = np.concatenate(S.masks)
    assert np.array_equal(u0, S.u0()) and not r[con].any()
    # (the rows of the last pass are not trivially right: lifted entries live there, in both fields)
    both = np.concatenate([last, last])
    assert np.count_nonzero(ref[both]) > 20
    if S.sigma[1] != 0.0:
        plain = R.System(S.kind, S.nd, S.cf, (0.0, 0.0), S.masks, S.g).rhs()
        assert np.count_nonzero((ref != plain) & both) > 0    # ... and the shift's share of the lifting as well
    ones = np.ones(S.n)
    for f in (0, 1):
        d, da = S.diag(f), S.diag(f, True)
        z = ctx.pc_apply(f, _ffi.PC_JACOBI, ones)
        frac = float((abs(z - np.where(S.masks[f], 0.0, 1.0 / d)) / (BAR * da / (d * d))).max())
        worst[1] = max(worst[1], frac)
        if not frac <= 1.0:
            worst[2].append((f"{tag} inverse diagonal {f}", frac))


_sparse_cache = {}


def _sparse_reference(name, sigma):
    """Entry-wise reference blocks from transient_reference.matfree_scalar_matrices, one mesh at a time."""
    c = _case(name)
    if _sparse_cache.get("name") != name:
        _sparse_cache.clear()
        nd = c["nd"]
        _sparse_cache.update(name=name, KM=T.matfree_scalar_matrices(c["kind"], nd[0], nd[1], nd[2] if len(nd) == 3 else 0))
    K, M = _sparse_cache["KM"]
    return T.shifted_blocks(K, M, CF, sigma, c["masks"], c["g"])[:4]


def _check_entries(tag, ctx, name, sigma):
    worst = 0.0
    for w, ref in zip(("A11", "A22", "A12", "A21"), _sparse_reference(name, sigma)):
        got = ctx.csr(MATS[w])
        err = abs(got - ref).max() / abs(ref).max()
        worst = max(worst, err)
        assert err <= VAL_TOL, (tag, w, err)
    return worst


@pytest.mark.parametrize("case,opts", RUNS, ids=[f"{c}-{s}" for c, s in RUNS])
def test_assembly_past_the_launch_caps(gpu_ctx_factory, case, opts):
    """Per case: the path and its passes from the restated rules; products (four blocks and the monolithic matrix, three vectors),
    right-hand side with lifting, inverse diagonals and, on quadrilaterals and hexahedra, the entry-wise export of the assembly with
    the dominant shift; products, right-hand side and inverse diagonals again after a second assembly with (0, 31); sigma = (0, 0)
    through the shifted entry point against pph_assemble_dpp bit for bit.

    What this case found (tests/README_asm_scale.md): with the reference-element table of k_asm_tile summed over rounded Gauss
    points, hex128x64x64-shifted-xmap missed the bound at 1.10 in one product (A11 of the (0, 31) assembly times the last-pass
    vector) - on 128 x 64 x 64 cells the directional terms of a stiffness entry cancel exactly for the corner pairs that differ in y
    and z, and seven rows of that product have a bound that rests on the mass share of such entries alone.  The table now holds
    the integrals in closed form, the terms cancel to 0 as they do in the reference, and the case is at 0.006."""
    t0 = time.time()
    c = _case(case)
    kind, nd, n = c["kind"], c["nd"], c["n"]
    options, shifted, path, xmap = (SIMPLEX_SETS if kind in (R.TRI, R.TET) else OPTION_SETS)[opts]
    od = dict(options)
    sigma = R.dominant_sigma(CF, nd[0]) if shifted else (0.0, 0.0)
    assert sigma[0] != sigma[1] or not shifted
    # which side of the thresholds: the path this context takes and more than one pass in it, with a constrained interior node
    # of field 1 in the last pass
    assert R.assembly_path(kind, n, not shifted, od.get("asm_node", 1), od.get("asm_tile", 1), od.get("op_format", 1) == 1) == path
    what, passes = _describe(kind, nd, path, xmap)
    assert passes >= 2
    if path == "two-pass":
        L = R.two_pass_launch(kind, nd)
        assert L["cell_passes"] >= 2 and L["node_passes"] >= 2
    last = R.last_pass_rows(kind, nd, path, xmap)
    inner1 = c["masks"][1] & ~c["masks"][0]
    assert 0 < np.count_nonzero(last) < n and np.count_nonzero(inner1 & last) >= 1
    lift_last = R.last_pass_rows(kind, nd, "step")
    assert R.step_rhs_launch(n)["passes"] >= 2 and np.count_nonzero(inner1 & lift_last) >= 1

    ctx = _context(gpu_ctx_factory, c, options)
    ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True, sigma=sigma)
    S = R.System(kind, nd, CF, sigma, c["masks"], c["g"])
    vectors = R.probe_vectors(n, last, 7)
    worst = [0.0, 0.0, []]
    tag = f"{case} {opts}"
    _check_products(tag, ctx, S, vectors, worst)
    _check_rhs_and_diagonal(tag, ctx, S, last | lift_last, worst)
    entries = None
    if kind in (R.QUAD, R.HEX):
        entries = _check_entries(tag, ctx, case, sigma)
    if shifted:
        # a later assembly is a new system: one field shifted ...
        S2 = R.System(kind, nd, CF, (0.0, 31.0), c["masks"], c["g"])
        ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True, sigma=(0.0, 31.0))
        _check_products(f"{tag} (0, 31)", ctx, S2, vectors, worst)
        _check_rhs_and_diagonal(f"{tag} (0, 31)", ctx, S2, last | lift_last, worst)
        # ... then none: pph_assemble_dpp_shifted with zeros is pph_assemble_dpp bit for bit (Context.assemble routes (0, 0) to
        # the plain entry point unless asked for the shifted one)
        ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True, sigma=(0.0, 0.0), shifted_entry=True)
        a = [ctx.spmv(MATS[w], np.concatenate([vectors[0], vectors[1]]) if w == "MONO" else vectors[0]) for w in R.WHICH] + list(ctx.rhs()) + \
            [ctx.pc_apply(f, _ffi.PC_JACOBI, vectors[1]) for f in (0, 1)]
        ctx.close()
        plain = _context(gpu_ctx_factory, c, options)
        plain.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True)
        b = [plain.spmv(MATS[w], np.concatenate([vectors[0], vectors[1]]) if w == "MONO" else vectors[0]) for w in R.WHICH] + list(plain.rhs()) + \
            [plain.pc_apply(f, _ffi.PC_JACOBI, vectors[1]) for f in (0, 1)]
        plain.close()
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    else:
        ctx.close()
    print(f"{tag}: {what}; worst fraction of the bound: products and right-hand sides {worst[0]:.3f}, inverse diagonals {worst[1]:.3f} "
          f"(bound {BAR:.2e} |A||x|)" + (f"; entries {entries:.2e} (bar {VAL_TOL:g})" if entries is not None else "") + f"; {time.time() - t0:.1f} s")
    assert not worst[2], worst[2]


# -- level operators ------------------------------------------------------------------------------------------------------
def test_level_operators_of_a_shifted_system(gpu_ctx_factory):
    """pph_launch_level_operators on a shifted system: level 1 (70 785 nodes) comes from the tile kernel, level 2 (9537) from
    the two-pass kernels, each with coefM = beta / mu + sigma_f of ITS field.  One application of the V-cycle per block against
    mg_cycle_reference.matfree_hierarchy, on the probing vectors of tests/test_mg_cycle_gpu.py (random; level 1; level 2)."""
    t0 = time.time()
    case = "hex128x64x64"
    c = _case(case)
    kind, nd, n = c["kind"], c["nd"], c["n"]
    levels = MC.level_nodes(kind, *nd)
    assert levels[:3] == [545025, 70785, 9537]
    assert R.assembly_path(kind, levels[0], False) == "tile" and R.assembly_path(kind, levels[1], False) == "tile"
    assert R.assembly_path(kind, levels[2], False) == "two-pass"
    assert R.tile_launch(kind, [q // 2 for q in nd])["passes"] == 1
    sigma = R.dominant_sigma(CF, nd[0])
    a, b, cc = CF.abc
    ctx = _context(gpu_ctx_factory, c)
    ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=False, sigma=sigma)
    for which, cK in ((0, a), (1, cc)):
        mask = c["masks"][which]
        lv = MC.matfree_hierarchy(kind, nd[0], nd[1], nd[2], cK, b + sigma[which], mask)
        other = MC.matfree_hierarchy(kind, nd[0], nd[1], nd[2], cK, b + sigma[1 - which], mask)
        vectors = MC.probe_vectors(lv, 11 + which)[:3]
        for ns in (1, 2):
            worst = (0.0, "")
            for name, r in vectors:
                ref = MC.apply_reference(lv, r, ns)
                z = ctx.pc_apply(which, _ffi.PC_MG, r, mg_smooth=ns)
                err = MC.rel_err(z, ref)
                worst = max(worst, (err, name))
                assert err <= MC.CYCLE_BOUND, (which, ns, name, err)
                assert not z[mask].any()
            off = MC.rel_err(MC.apply_reference(other, vectors[1][1], ns), MC.apply_reference(lv, vectors[1][1], ns))
            print(f"{case} level operators, block {which} mg_smooth {ns}: worst |z - ref| / |ref| = {worst[0]:.2e} ({worst[1]}), bound "
                  f"{MC.CYCLE_BOUND:.0e}; a hierarchy with the other field's shift: {off:.2e}")
            assert off > 1e3 * MC.CYCLE_BOUND
    ctx.close()
    print(f"{case} level operators: {time.time() - t0:.1f} s")


# -- step kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tri2048x1024", "hex128x64x64", "tet128"])
def test_step_rhs_past_one_pass_of_the_grid(gpu_ctx_factory, case):
    """k_step_rhs<KIND, false> in a second pass and beyond: the 3D index path (t32 / py, pxy * oz) and both simplex tables."""
    t0 = time.time()
    c = _case(case)
    kind, nd, n = c["kind"], c["nd"], c["n"]
    L = R.step_rhs_launch(n)
    assert L["grid"] == R.STEP_MAX_WG and L["passes"] >= 2 and T.step_kernel_loops(n)
    last = R.last_pass_rows(kind, nd, "step")
    assert np.count_nonzero(c["masks"][1] & ~c["masks"][0] & last) >= 1
    S = R.System(kind, nd, CF, (0.0, 0.0), c["masks"], c["g"])
    ctx = _context(gpu_ctx_factory, c)
    worst = [0.0, 0.0, []]
    rng = np.random.default_rng(23)
    tail = np.concatenate([last, last]) * rng.standard_normal(2 * n)
    for vi, p in enumerate((rng.standard_normal(2 * n), tail)):
        bdev = ctx.step_rhs(p, CF.k1, CF.k2, CF.beta, CF.mu)
        ref = S.step_rhs(p)
        _within(f"{case} step_rhs vector {vi}", bdev, ref, S.step_rhs(p, True), worst)
        con = np.concatenate(c["masks"])
        assert not bdev[con].any() and not np.any(np.signbit(bdev[con]))
        assert np.array_equal(bdev, ctx.step_rhs(p, CF.k1, CF.k2, CF.beta, CF.mu))
        assert np.count_nonzero(ref[np.concatenate([last, last])]) > 400
    ctx.close()
    print(f"{case}: k_step_rhs on {L['grid']} x 256 threads, {L['passes']} passes; worst fraction of the bound {worst[0]:.3f} "
          f"(bound {BAR:.2e} |A||p|); {time.time() - t0:.1f} s")
    assert not worst[2], worst[2]


def _cg_jacobi(rtol):
    cfg, _ = solver.translate_options(spar.CG_JACOBI_PARAMS, nonlinear=False)
    cfg.rtol, cfg.atol = rtol, 1e-300
    return cfg


STEP_RTOL = 1e-10


@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_two_steps_past_the_step_kernels_caps(gpu_ctx_factory, theta):
    """pph_transient_begin + two pph_transient_steps of one step each on hex 128x64x64 (CG + Jacobi, rtol 1e-10): k_step_constrain
    and k_step_update + k_step_sum run over 1 090 050 entries on 2048 workgroups (3 passes, all 2048 partial-sum slots live).
    S_f / dt is the dominant shift, so Sigma M / dt dominates theta A and CG + Jacobi converges in a few dozen iterations."""
    t0 = time.time()
    case = "hex128x64x64"
    c = _case(case)
    kind, nd, n = c["kind"], c["nd"], c["n"]
    L = R.step_update_launch(n)
    assert L["grid"] == R.STEP_MAX_WG and L["passes"] == 3
    dt = 1.0 / (10.0 * nd[0] ** 2)
    storage = (CF.k1 / CF.mu, CF.k2 / CF.mu)
    sig = (storage[0] / dt, storage[1] / dt)
    assert np.allclose(sig, R.dominant_sigma(CF, nd[0]), rtol=1e-14)
    con = np.concatenate(c["masks"])
    gg = np.concatenate(c["g"])
    i, j, k = R.node_ijk(nd)
    x, y, z = i / nd[0], j / nd[1], k / nd[2]
    p0 = np.concatenate([np.cos(2.0 * x) + y, 0.3 + 0.5 * np.sin(3.0 * z)]) + 0.05 * np.random.default_rng(2).standard_normal(2 * n)
    cfg = _cg_jacobi(STEP_RTOL)
    ctx = _context(gpu_ctx_factory, c)
    ctx.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, storage, theta, dt)
    Ssteady = R.System(kind, nd, CF, (0.0, 0.0), c["masks"], c["g"])
    Sstep = R.System(kind, nd, T.Coefs(theta * CF.k1, theta * CF.k2, theta * CF.beta, CF.mu), sig, c["masks"], c["g"])
    dinv = 1.0 / np.concatenate([Sstep.diag(0), Sstep.diag(1)])
    drift = R.residual_drift(kind, theta)
    p = p0.copy()
    prev = np.where(con, gg, p0)
    for s in range(2):
        done, infos, norms = ctx.transient_steps(cfg, p, 1)
        assert done == 1 and infos[0].converged and infos[0].iterations > 0
        assert np.array_equal(p[con], gg[con])
        bref = Ssteady.step_rhs(prev)
        d = p - prev
        for what, got, vec in (("||b_s||", norms[0, 0], bref), ("||p^{s+1} - p^s||", norms[0, 1], d)):
            want = float(np.linalg.norm(vec))
            rel, tol = R.norm_check(got, vec)     # (on the squared sums, as for the error norms)
            print(f"{case} theta {theta} step {s}: {what} {got:.15e}, reference {want:.15e}, relative difference of the squares {rel:.2e} (bound {tol:.1e})")
            assert rel <= tol, (what, s, rel, tol)
        r = Sstep.apply("MONO", d) - bref
        r[con] = 0.0
        res, bn = float(np.linalg.norm(dinv * r)), float(np.linalg.norm(dinv * bref))
        bound = (STEP_RTOL + 100.0 * drift) * bn
        print(f"{case} theta {theta} step {s}: ||D^-1 r|| = {res:.3e} = {res / bn:.2e} ||D^-1 b||, bound {bound / bn:.2e} ||D^-1 b|| (rtol {STEP_RTOL:g} + 100 x "
              f"drift {drift:.1e}); {infos[0].iterations} iterations")
        assert res <= bound
        prev = p.copy()
    ctx.close()
    print(f"{case} theta {theta}: {L['grid']} workgroups, {L['passes']} passes over 2n; {time.time() - t0:.1f} s")


# -- the node kernel past its grid ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.UNSHIFTED_ONLY))
def test_node_kernel_past_its_grid(gpu_ctx_factory, case):
    """k_asm_node2 in its two split launches with more than 16 384 x 256 rows: products, right-hand side and inverse diagonals
    of the default (unshifted) assembly - and the monolithic matrix built from the node kernel's stencil-ELL blocks
    (pph_ensure_csr_blocks, k_mono_rowptr and k_mono_fill in several passes) as a product under the same row-wise bound."""
    t0 = time.time()
    c = _case(case)
    kind, nd, n = c["kind"], c["nd"], c["n"]
    assert R.assembly_path(kind, n, True) == "node"
    L = R.node_launch(n)
    assert L["grid"] == R.NODE_MAX_WG and L["passes"] == 2 and L["split"] == 1 and n > 64 * L["windows_per_launch"]
    Lm = R.mono_launch(n)
    assert n > 4194304 and Lm["rowptr_grid"] == 4096 and Lm["rowptr_passes"] >= 5 and Lm["fill_grid"] == 4096 and Lm["fill_passes"] >= 33
    last = R.last_pass_rows(kind, nd, "node")
    assert np.count_nonzero(c["masks"][1] & ~c["masks"][0] & last) >= 1
    ctx = _context(gpu_ctx_factory, c)
    ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True)
    S = R.System(kind, nd, CF, (0.0, 0.0), c["masks"], c["g"])
    vectors = R.probe_vectors(n, last, 9)
    worst = [0.0, 0.0, []]
    two = vectors[:1] + vectors[2:]
    _check_products(case, ctx, S, two, worst, ("A11", "A22", "A12", "A21"))
    t1 = time.time()
    _check_products(case, ctx, S, two, worst, ("MONO",))     # ([v0; vL] and [vL; v0]: the pieces of the block products)
    t_mono = time.time() - t1
    _check_rhs_and_diagonal(case, ctx, S, last, worst)
    ctx.close()
    what, _ = _describe(kind, nd, "node", 0)
    print(f"{case}: {what}; k_mono_rowptr {Lm['rowptr_passes']} passes, k_mono_fill {Lm['fill_passes']}; worst fraction of the bound: products "
          f"(monolithic included) and right-hand side {worst[0]:.3f}, inverse diagonals {worst[1]:.3f} (bound {BAR:.2e} |A||x|); "
          f"{time.time() - t0:.1f} s, of which the monolithic products {t_mono:.1f} s")
    assert not worst[2], worst[2]
    _case_cache.clear()
    R.clear_pieces()
