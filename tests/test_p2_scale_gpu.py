"""Degree-2 (Q2 / P2) device kernels past the sizes where they leave their simplest branch, against fp64 restatements
(tests/p2_matfree.py for assembly, products and error norms, tests/pmg_restatement.py for the p-multigrid cycle,
tests/p2_restatement.py for ILU(0)).  Every test asserts that its mesh is past the threshold it targets; the thresholds
are restated below from the kernels' launch code, so that a kernel change that moves one makes the test say so.  Large
contexts are closed at the end of each test (the session fixture would keep them to the end of the run)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import p2_matfree as F  # noqa: E402
import p2_restatement as R  # noqa: E402
import pmg_restatement as PM  # noqa: E402

from perphil_amd import _ffi, solver_parameters as spar  # noqa: E402
from perphil_amd.solver import translate_options  # noqa: E402

pytestmark = pytest.mark.gpu

K1, K2, BETA, MU = 1.0, 0.01, 1.0, 1.0

# pph_p2.hip, p2_grid: at most 4096 workgroups of 256 lanes for k_p2_coords / _dofmap / _row_count / _row_fill / _km
P2_GRID_LANES = 4096 * 256
# pph_post.hip, norms_mms / pph_error_norms_sampled: grid = min(ceil(cells / 256), 2048) workgroups of 256 lanes
NORM_GRID_LANES = 2048 * 256
# pph_pmg.hip, pmg_cap / pmg_grid: LDS doubles per tile and 256 CUs x (160 KiB / (8 cap + 512 B)) workgroups, a multiple of 8
PMG_CAP = {64: 1664, 32: 4096, 16: 2048}
# pph_ilu.hip: the triangular sweeps are captured into a graph only up to 4096 levels
ILU_GRAPH_LEVELS = 4096
# pph_p2.hip, pph_p2_mesh: degree-2 nodes per field < 2^30 - 1, entries of the scalar block < 2^31 - 1
NODE_LIMIT, NNZ_LIMIT = 2 ** 30 - 1, 2 ** 31 - 1


def pmg_workgroups(rows, R_):
    cap = 256 * (160 * 1024 // (PMG_CAP[R_] * 8 + 512))
    g = min(-(-rows // R_), cap)
    return max((g + 7) // 8 * 8, 8)


def _data(kind, nx, ny, nz, variant=0):
    """Dirichlet nodes and non-trivial data; variant 1: every side except x = 1 (a natural boundary there)."""
    X = R.coords(kind, nx, ny, nz)
    b = R.boundary_nodes(kind, nx, ny, nz)
    if variant == 1:
        b = b[X[b, 0] < 1.0 - 1e-12]
        return b, 1.0 + X[b, 1] ** 2, np.cos(X[b, 0]) - X[b, -1]
    return b, np.exp(X[b, 0]) * np.sin(3 * X[b, 1]), np.cos(2 * X[b, 0]) + X[b, -1]


def _new_ctx(gpu_ctx_factory, kind, nx, ny, nz):
    ctx = gpu_ctx_factory()
    ctx.mesh_build_lagrange(R.dim_of(kind), kind, nx, ny, nz, 2)
    return ctx


def _setup(ctx, kind, nx, ny, nz, variant=0, monolithic=True):
    b, g1, g2 = _data(kind, nx, ny, nz, variant)
    ctx.set_dirichlet(0, b, g1)
    ctx.set_dirichlet(1, b, g2)
    ctx.assemble(K1, K2, BETA, MU, monolithic=monolithic)
    mask = np.zeros(ctx.n, bool)
    mask[b] = True
    return b, g1, g2, mask


def _csr_sizes(ctx, which):
    import ctypes as C

    nrows, nnz = C.c_int64(), C.c_int64()
    ctx._check(_ffi.lib.pph_csr_sizes(ctx._h, which, C.byref(nrows), C.byref(nnz)))
    return nrows.value, nnz.value


# ----------------------------------------------------------------------------------------------------------------------
# a. assembly and products past the grid-stride cap of pph_p2.hip
# ----------------------------------------------------------------------------------------------------------------------
SCALE = {"quad1100x1000": (R.QUAD, 1100, 1000, 0), "tri1100x1000": (R.TRI, 1100, 1000, 0), "hex64": (R.HEX, 64, 64, 64),
         "tet64x64x48": (R.TET, 64, 64, 48), "quad512": (R.QUAD, 512, 512, 0)}
SPMV_WHICH = {"K": _ffi.MAT_K, "M": _ffi.MAT_M, "A11": _ffi.MAT_A11, "A22": _ffi.MAT_A22, "A12": _ffi.MAT_A12,
              "A21": _ffi.MAT_A21, "MONO": _ffi.MAT_MONO}


@pytest.mark.parametrize("name", list(SCALE))
def test_assembly_and_products_past_grid_stride(gpu_ctx_factory, name):
    """Cell->dof map and coordinates exact, pattern size exact, K / M / A11 / A22 / A12 / A21 / MONO products of three
    random vectors and the lifted right-hand side row by row within c u mag_i (p2_matfree.spmv_bound_factor), u0 exact;
    whole boundary constrained, then every side but x = 1."""
    kind, nx, ny, nz = SCALE[name]
    d = R.dim_of(kind)
    n = R.n_nodes(kind, nx, ny, nz)
    nbox = nx * ny * (nz if d == 3 else 1)
    print(f"{name}: {n} degree-2 nodes, {nbox} boxes vs {P2_GRID_LANES} lanes of the capped p2_grid "
          f"({n - P2_GRID_LANES} nodes in the grid-stride passes)")
    assert n > P2_GRID_LANES
    if name == "quad1100x1000":
        assert nbox > P2_GRID_LANES          # k_p2_dofmap's second pass too
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    try:
        assert ctx.n == n and ctx.nnzb == F.nnz_closed_form(kind, nx, ny, nz)
        assert np.array_equal(ctx.dofmap(), F.dofmap_fast(kind, nx, ny, nz))
        assert np.array_equal(ctx.coords(), R.coords(kind, nx, ny, nz))
        op = F.Operator(kind, nx, ny, nz)
        mrow = F.max_row(kind)
        worst = {}
        for variant in (0, 1):
            b, g1, g2, mask = _setup(ctx, kind, nx, ny, nz, variant)
            nnz = F.nnz_closed_form(kind, nx, ny, nz)
            assert _csr_sizes(ctx, _ffi.MAT_K) == (n, nnz) and _csr_sizes(ctx, _ffi.MAT_A11) == (n, nnz)
            assert _csr_sizes(ctx, _ffi.MAT_MONO) == (2 * n, 4 * nnz)
            G1, G2 = np.zeros(n), np.zeros(n)
            G1[b], G2[b] = g1, g2
            r_ref, r_mag, u_ref = F.lift(kind, (nx, ny, nz), mask, G1, G2, K1, K2, BETA, MU, op=op)
            r, u0 = ctx.rhs()
            assert np.array_equal(u0, u_ref)
            c = F.spmv_bound_factor(2 * mrow, d)
            e = F.row_excess(r, r_ref, r_mag, c)
            worst[("rhs", variant)] = e
            assert e <= 1.0, (variant, "rhs", e)
            rng = np.random.default_rng(100 + variant)
            for _ in range(3):
                x1, x2 = rng.standard_normal(n), rng.standard_normal(n)
                ref = F.apply_blocks(kind, (nx, ny, nz), mask, x1, x2, K1, K2, BETA, MU, op=op)
                for w, which in SPMV_WHICH.items():
                    x = {"A22": x2, "A12": x2, "MONO": np.concatenate([x1, x2])}.get(w, x1)
                    y = ctx.spmv(which, x)
                    c = F.spmv_bound_factor(2 * mrow if w == "MONO" else mrow, d)
                    e = F.row_excess(y, ref[w][0], ref[w][1], c)
                    worst[(w, variant)] = max(worst.get((w, variant), 0.0), e)
                    assert e <= 1.0, (variant, w, e)
        for key, e in sorted(worst.items()):
            print(f"  {key}: worst |y - y_ref|_i / (c u mag_i) = {e:.3e} (bound 1)")
        if name == "quad512":
            # full export: every row's length and columns
            A = ctx.csr(_ffi.MAT_K)
            rowptr, col = F.pattern_fast(kind, nx, ny, nz)
            assert np.array_equal(np.diff(A.indptr), F.row_lengths(kind, nx, ny, nz))
            assert np.array_equal(A.indptr, rowptr) and np.array_equal(A.indices, col)
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------------------------------------
# b. pph_pmg with several tiles per workgroup
# ----------------------------------------------------------------------------------------------------------------------
PMG_SCALE = {"quad256": (R.QUAD, 256, 256, 0, 64), "tri256x200": (R.TRI, 256, 200, 0, 64),
             "hex20x20x18_r32": (R.HEX, 20, 20, 18, 32), "hex20x20x18_r16": (R.HEX, 20, 20, 18, 16),
             "tet20x20x18_r32": (R.TET, 20, 20, 18, 32), "tet20x20x18_r16": (R.TET, 20, 20, 18, 16)}
_LEVELS = {}


def _levels(kind, nx, ny, nz, ck, mask, variant):
    key = (kind, nx, ny, nz, ck, variant)
    if key not in _LEVELS:
        for k in [k for k in _LEVELS if k[:4] != key[:4] or k[5] != variant]:
            del _LEVELS[k]                     # keep the two blocks of the current mesh and Dirichlet set only
        _LEVELS[key] = PM.build_levels(kind, nx, ny, nz, ck, BETA / MU, mask)
    return _LEVELS[key]


def _permuted_cycle(lv, b, steps, seed):
    """The restated cycle with the degree-2 level's rows / columns permuted (another summation order), permuted back."""
    top = lv[0]
    n = b.size
    p = np.random.default_rng(seed).permutation(n)
    A = top.A.tocsr()[p][:, p].tocsr()
    t2 = PM.G.Level(A, top.dinv[p], top.mask[p], top.lam)
    t2.P = top.P.tocsr()[p]
    z = PM.cycle([t2] + lv[1:], b[p], steps)
    out = np.empty(n)
    out[p] = z
    return out


def _check_cycle(ctx, kind, nx, ny, nz, mask, seed, variant, drift=False):
    rng = np.random.default_rng(seed)
    worst = 0.0
    for which, ck in ((0, K1 / MU), (1, K2 / MU)):
        lv = _levels(kind, nx, ny, nz, ck, mask, variant)
        for ns in (1, 2):
            r = rng.standard_normal(ctx.n)
            rm = r.copy()
            rm[mask] = 0.0
            ref = PM.cycle(lv, rm, ns)
            if drift and which == 0 and ns == 2:
                dr = F.rel_max_error(_permuted_cycle(lv, rm, ns, seed), ref)
                print(f"  restatement drift (rows permuted and back): {dr:.3e} (reported when above 1e-11)")
                if dr > 1e-11:
                    print("  NOTE: the restatement drifts from itself by more than 1e-11 at this size")
            ctx.set_option("pmg_fused", 1)
            z = ctx.pc_apply(which, _ffi.PC_PMG, r, mg_smooth=ns)
            err = F.rel_max_error(z, ref)
            ctx.set_option("pmg_fused", 0)
            zg = ctx.pc_apply(which, _ffi.PC_PMG, r, mg_smooth=ns)
            ctx.set_option("pmg_fused", 1)
            errg = F.rel_max_error(zg, ref)
            fg = F.rel_max_error(z, zg)
            print(f"  block {which} mg_smooth {ns}: fused {err:.3e}, generic {errg:.3e} (bound 1e-10); "
                  f"fused vs generic {fg:.3e} (bound 1e-12)")
            worst = max(worst, err, errg)
            assert err <= 1e-10 and errg <= 1e-10
            assert fg <= 1e-12
            assert not z[mask].any() and not zg[mask].any()                     # exact zeros on constrained dofs
            assert np.array_equal(z, ctx.pc_apply(which, _ffi.PC_PMG, r, mg_smooth=ns))   # bitwise repeatable
    return worst


@pytest.mark.parametrize("name", list(PMG_SCALE))
def test_pmg_cycle_multi_tile(gpu_ctx_factory, name):
    """The cycle against pmg_restatement.cycle where a workgroup of k_pmg_level0 takes several tiles (the LDS products
    and row offsets of a tile are rewritten after the second barrier).  The restatement's own drift at these sizes (the
    degree-2 level's rows permuted and permuted back) is printed by every case."""
    kind, nx, ny, nz, Rt = PMG_SCALE[name]
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    try:
        if R.dim_of(kind) == 3:
            ctx.set_option("pmg_tile_rows", Rt)
        rows = ctx.n
        wg = pmg_workgroups(rows, Rt)
        tpx = -(-(-(-rows // Rt)) // 8)
        print(f"{name}: {rows} rows, {-(-rows // Rt)} tiles of {Rt}: {tpx} tiles per XCD vs {wg // 8} workgroups per XCD")
        assert tpx > wg // 8
        _, _, _, mask = _setup(ctx, kind, nx, ny, nz, monolithic=False)
        _check_cycle(ctx, kind, nx, ny, nz, mask, seed=21, variant=0, drift=True)
        if name == "hex20x20x18_r16":
            _, _, _, mask = _setup(ctx, kind, nx, ny, nz, variant=1, monolithic=False)
            print(" natural boundary at x = 1:")
            _check_cycle(ctx, kind, nx, ny, nz, mask, seed=22, variant=1)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", [R.QUAD, R.TRI, R.HEX, R.TET])
@pytest.mark.parametrize("cells", [1, 2])
def test_pmg_cycle_degenerate_meshes(gpu_ctx_factory, kind, cells):
    """One or two cells per direction, whole boundary constrained: one free degree-2 dof or 3^d of them, and a CG-1 level
    that is all (one cell) or all but one node (two cells) Dirichlet."""
    nz = cells if R.dim_of(kind) == 3 else 0
    ctx = _new_ctx(gpu_ctx_factory, kind, cells, cells, nz)
    try:
        _, _, _, mask = _setup(ctx, kind, cells, cells, nz, monolithic=False)
        assert int((~mask).sum()) == (1 if cells == 1 else 3 ** R.dim_of(kind))
        print(f"kind {kind}, {cells} cell(s) per direction: {int((~mask).sum())} free dofs")
        _check_cycle(ctx, kind, cells, cells, nz, mask, seed=23, variant=0)
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------------------------------------
# c. degree-2 error norms against norms_reference
# ----------------------------------------------------------------------------------------------------------------------
NORM_MESHES = {"quad800x700": (R.QUAD, 800, 700, 0), "tri600x500": (R.TRI, 600, 500, 0),
               "tet48x48x40": (R.TET, 48, 48, 40), "hex40x30x20": (R.HEX, 40, 30, 20)}
NQ = {2: 6, 3: 4}          # Gauss points per direction (3D: 4, to keep the host reference within seconds)


def _check_norms(ctx, kind, dims, nodal, field, label, chunks=(7, 1000, -1, 0)):
    """All three sources against norms_reference, each squared norm within norms_bound."""
    import torch

    d = R.dim_of(kind)
    nq = NQ[d]
    ncell = ctx.ncell
    p, g = F.mms_exact(field, d, K1, K2, BETA, MU)
    ref = F.norms_reference(kind, dims, nodal, p, g, nq)
    b_l2, b_h1, L = F.norms_bound(ref, kind, ncell, nq)
    grid = min(-(-ncell // 256), 2048)
    print(f"{label}: {ncell} cells vs {NORM_GRID_LANES} lanes of the capped grid ({grid} workgroups); "
          f"ref |e|^2 = {ref['l2']:.6e}, |e|_1^2 = {ref['h1']:.6e}; L = {L}")

    def check(tag, l2, h1, bl2=b_l2, bh1=b_h1):
        e1, e2 = abs(l2 * l2 - ref["l2"]), abs(h1 * h1 - ref["h1"])
        print(f"  {tag}: |dL2^2| {e1:.3e} (bound {bl2:.3e}), |dH1^2| {e2:.3e} (bound {bh1:.3e})")
        assert F.norms_excess((l2 * l2, h1 * h1), ref, (bl2, bh1)) <= 1.0, tag
        return l2 * l2, h1 * h1

    check("error_norms_mms", *ctx.error_norms_mms(field, nodal, K1, K2, BETA, MU, nq=nq))
    t = torch.as_tensor(nodal, device=f"cuda:{ctx.device}")
    check("error_norms_mms_device", *ctx.error_norms_mms_device(field, t, K1, K2, BETA, MU, nq=nq))
    got = []
    for ch in chunks:
        cc = ncell - 1 if ch == -1 else (ncell if ch == 0 else ch)
        calls = -(-ncell // cc)
        # the longest chain: one call's (min(cc, ncell) cells) plus the host's sum over the calls
        gcc = min(-(-min(cc, ncell) // 256), 2048)
        Lc = -(-min(cc, ncell) // (gcc * 256)) * nq ** d + 2304 + calls
        bl2 = F.U * (2 * (R.nodes_per_cell(kind) + 20) * ref["S_l2"] + Lc * ref["l2"])
        bh1 = F.U * (2 * (R.nodes_per_cell(kind) + 20) * ref["S_h1"] + Lc * ref["h1"])
        got.append(check(f"error_norms_sampled chunk_cells {cc} (L = {Lc})",
                         *ctx.error_norms_sampled(nodal, p, g, nq=nq, chunk_cells=cc), bl2, bh1) + (bl2, bh1))
    for a in got:
        for b in got:
            assert abs(a[0] - b[0]) <= max(a[2], b[2]) and abs(a[1] - b[1]) <= max(a[3], b[3])
    return ref


@pytest.mark.parametrize("name", list(NORM_MESHES))
def test_error_norms_against_reference(gpu_ctx_factory, name):
    """Interpolant of the manufactured pressure plus a seeded 10 % perturbation (no cancellation in u_h - p); the
    quadrature points of every cell to 4 u max|x|."""
    kind, nx, ny, nz = NORM_MESHES[name]
    d = R.dim_of(kind)
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    try:
        if name != "hex40x30x20":
            assert ctx.ncell > NORM_GRID_LANES
        X = R.coords(kind, nx, ny, nz)
        p, _ = F.mms_exact(0, d, K1, K2, BETA, MU)
        pv = p(X)
        nodal = pv + 0.1 * np.abs(pv).max() * np.random.default_rng(31).uniform(-1.0, 1.0, pv.size)
        _check_norms(ctx, kind, (nx, ny, nz), nodal, 0, name)
        nq = NQ[d]
        step = 1 << 16
        worst, xmax = 0.0, 0.0
        for c0 in range(0, ctx.ncell, step):
            cnt = min(step, ctx.ncell - c0)
            xq = ctx.quadrature_points(nq, c0, cnt)
            ref = F.norms_reference(kind, (nx, ny, nz), nodal, lambda Y: Y[:, 0], lambda Y: Y, nq,
                                    cell_range=(c0, c0 + cnt), want_points=True)["points"]
            worst, xmax = max(worst, float(abs(xq - ref).max())), max(xmax, float(abs(ref).max()))
        print(f"  quadrature points: max |x - x_ref| = {worst:.3e} (bound 4u max|x| = {4 * F.U * xmax:.3e})")
        assert worst <= 4 * F.U * xmax
    finally:
        ctx.close()


@pytest.mark.parametrize("kind,nx,ny,nz", [(R.QUAD, 48, 40, 0), (R.TET, 10, 9, 8)])
def test_error_norms_of_a_solution(gpu_ctx_factory, kind, nx, ny, nz):
    """An actual GMRES + ILU(0) solution with the manufactured Dirichlet data: u_h - p is a cancellation there, and the
    bound (built from |u_h| and |p|) widens with it."""
    d = R.dim_of(kind)
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    try:
        X = R.coords(kind, nx, ny, nz)
        b = R.boundary_nodes(kind, nx, ny, nz)
        p1, _ = F.mms_exact(0, d, K1, K2, BETA, MU)
        p2, _ = F.mms_exact(1, d, K1, K2, BETA, MU)
        ctx.set_dirichlet(0, b, p1(X[b]))
        ctx.set_dirichlet(1, b, p2(X[b]))
        ctx.assemble(K1, K2, BETA, MU, monolithic=True)
        cfg, _ = translate_options({**spar.GMRES_ILU_PARAMS, "ksp_rtol": 1e-12, "ksp_atol": 1e-30})
        x, info, _ = ctx.solve(cfg)
        assert info.converged
        x = x.copy()
        for field in (0, 1):
            _check_norms(ctx, kind, (nx, ny, nz), x[field * ctx.n:(field + 1) * ctx.n].copy(), field,
                         f"kind {kind} {nx}x{ny}x{nz} GMRES + ILU field {field}", chunks=(7, 1000, -1, 0))
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------------------------------------
# d. ILU(0) at degree 2
# ----------------------------------------------------------------------------------------------------------------------
ILU_MESHES = {"quad21x13": (R.QUAD, 21, 13, 0), "tri17x12": (R.TRI, 17, 12, 0), "hex6x4x5": (R.HEX, 6, 4, 5),
              "tet5x4x6": (R.TET, 5, 4, 6)}


def ilu_levels(kind, nx, ny, nz):
    """Levels of the degree-2 sweeps (pph_ilu.hip): i + 3 j + 9 k, 0 .. max."""
    px, py, pz = R.lattice_dims(kind, nx, ny, nz)
    return (px - 1) + 3 * (py - 1) + 9 * (pz - 1) + 1


@pytest.mark.parametrize("name", list(ILU_MESHES))
def test_ilu0_degree2(gpu_ctx_factory, name):
    """pc_apply(PC_ILU) on both blocks against R.ilu0 / R.ilu_apply within max(100 delta, 1e-13) |z_ref|_inf, where delta is
    the restatement's own discrepancy from its longdouble run; "use_graphs" 0 bitwise equal to the graph replay; GMRES +
    ILU(0) iteration counts on the monolithic system equal R.gmres_left."""
    kind, nx, ny, nz = ILU_MESHES[name]
    ctx = _new_ctx(gpu_ctx_factory, kind, nx, ny, nz)
    try:
        nl = ilu_levels(kind, nx, ny, nz)
        print(f"{name}: {ctx.n} nodes, {nl} levels (graph capture up to {ILU_GRAPH_LEVELS}; the no-graph path by "
              f"\"use_graphs\" 0)")
        assert nl <= ILU_GRAPH_LEVELS          # so that use_graphs 1 replays a graph and 0 does not
        b, g1, g2, mask = _setup(ctx, kind, nx, ny, nz)
        rng = np.random.default_rng(41)
        for which, mat in ((0, _ffi.MAT_A11), (1, _ffi.MAT_A22)):
            A = ctx.csr(mat)
            r = rng.standard_normal(ctx.n)
            rm = r.copy()
            rm[mask] = 0.0
            ref = R.ilu_apply(R.ilu0(A), rm)
            ld = F.ilu_apply(F.ilu0(A, np.longdouble), rm.astype(np.longdouble))
            delta = float(np.max(np.abs(ref - ld)) / np.max(np.abs(ld)))
            tol = max(100 * delta, 1e-13) * abs(ref).max()
            ctx.set_option("use_graphs", 1)
            z = ctx.pc_apply(which, _ffi.PC_ILU, r)
            ctx.set_option("use_graphs", 0)
            zn = ctx.pc_apply(which, _ffi.PC_ILU, r)
            ctx.set_option("use_graphs", 1)
            err = abs(z - ref).max()
            print(f"  block {which}: delta = {delta:.3e}, |z - z_ref| = {err:.3e} (bound {tol:.3e}), "
                  f"graph == no graph: {np.array_equal(z, zn)}")
            assert err <= tol
            assert np.array_equal(z, zn)
        Kr, Mr = R.assemble_KM(kind, nx, ny, nz)
        A11, A22, A12, A21, rhs, _ = R.eliminate(Kr, Mr, b, g1, g2, K1, K2, BETA, MU)
        A = R.monolithic(A11, A22, A12, A21)
        cfg, _ = translate_options({**spar.GMRES_ILU_PARAMS, "ksp_rtol": 1e-10, "ksp_atol": 1e-30})
        _, info, _ = ctx.solve(cfg)
        fac = R.ilu0(ctx.csr(_ffi.MAT_MONO))
        _, its = R.gmres_left(A, rhs, lambda v: R.ilu_apply(fac, v), rtol=1e-10, atol=1e-30)
        print(f"  GMRES + ILU(0): device {info.iterations}, restatement {its}")
        assert info.iterations == its
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------------------------------------
# e. int32 limits
# ----------------------------------------------------------------------------------------------------------------------
def smallest_hex_past_nnz_limit():
    """Smallest N with (8 N + 1)^3 > 2^31 - 1 (the Q2 hex N^3 scalar block, p2_matfree.nnz_closed_form)."""
    N = 1
    while F.nnz_closed_form(R.HEX, N, N, N) <= NNZ_LIMIT - 1:
        N += 1
    return N


@pytest.mark.parametrize("case", ["quad16384_nodes", "hex_nnz"])
def test_int32_limits_refuse_cleanly(gpu_ctx_factory, case):
    ctx = gpu_ctx_factory()
    try:
        if case == "quad16384_nodes":
            kind, N = R.QUAD, 16384
            n = R.n_nodes(kind, N, N)
            print(f"Q2 quad {N}^2: {n} nodes vs the limit {NODE_LIMIT}")
            assert n >= NODE_LIMIT
            with pytest.raises(ValueError, match="int32"):
                ctx.mesh_build_lagrange(2, kind, N, N, 0, 2)
        else:
            N = smallest_hex_past_nnz_limit()
            nnz = F.nnz_closed_form(R.HEX, N, N, N)
            print(f"Q2 hex {N}^3: {nnz} entries vs the limit {NNZ_LIMIT} ({N - 1}^3: "
                  f"{F.nnz_closed_form(R.HEX, N - 1, N - 1, N - 1)})")
            assert nnz >= NNZ_LIMIT and F.nnz_closed_form(R.HEX, N - 1, N - 1, N - 1) < NNZ_LIMIT
            with pytest.raises(ValueError, match="int32"):
                ctx.mesh_build_lagrange(3, R.HEX, N, N, N, 2)
        # the same context builds and assembles a small mesh
        kind, nx, ny, nz = R.TET, 3, 4, 2
        ctx.mesh_build_lagrange(3, kind, nx, ny, nz, 2)
        b, g1, g2, mask = _setup(ctx, kind, nx, ny, nz)
        Kr, Mr = R.assemble_KM(kind, nx, ny, nz)
        A11, A22, A12, A21, rhs, u0 = R.eliminate(Kr, Mr, b, g1, g2, K1, K2, BETA, MU)
        for which, ref in [(_ffi.MAT_K, Kr), (_ffi.MAT_M, Mr), (_ffi.MAT_A11, A11), (_ffi.MAT_A12, A12)]:
            A = ctx.csr(which)
            assert abs(A - ref).max() <= 1e-12 * abs(ref).max()
        r, u = ctx.rhs()
        assert abs(r - rhs).max() <= 1e-12 * max(abs(rhs).max(), 1.0) and np.array_equal(u, u0)
    finally:
        ctx.close()

