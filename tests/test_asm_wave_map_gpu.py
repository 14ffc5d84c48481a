"""The node assembly kernel's two wave maps (option asm_node_lines: 1 windows that follow the grid lines, 0 waves of 64
aligned rows) store the same bits.

Both forms of the kernel are one source with pinned roundings, so moving an interior row from the general to the
straight-line launch must change nothing.  On ONE context, assembled with asm_node_lines 0, 1, 0, 2 in turn (from the second
assembly on they run the dictionary check fused into the kernel, once per map), these are compared bit for bit:

  * the four fine blocks through the CSR export (what test_node_assembly_kernel_equals_tile_kernel reads), the right-hand
    side and u0;
  * the inverse diagonals: z = pc_apply(PC_JACOBI) of a vector of ones;
  * every multigrid level - the levels have no export of their own: z = pc_apply(PC_MG) of random vectors is a function of
    every level's stored operators, inverse diagonals and spectral bounds (the smoother weights), for both blocks;
  * the state of the row dictionaries (usable / refused, classes), and on one case the Picard solve.

asm_node_split_min is lowered so that the small boxes here - and their first coarse levels - run in two launches.  The boxes
have 33 / 34 nodes per line (no window fits: both maps must still agree), 73 / 74 (one window per line, odd / even line
length: the parity of a line's first row alternates or not), 141 and 161 (several windows, the last one overlapping; a first
coarse level of 71 / 81 nodes per line with windows of its own).  One case asserts coverage: the outputs are filled with NaNs
before the kernel runs (option asm_poison), so a row that neither launch stores fails the comparison and the NaN scan.
"""
import numpy as np
import pytest

from oracle import dpp_oracle as o

pytestmark = pytest.mark.gpu

P = o.Params(k1=1.0, k2=0.01, beta=1.0, mu=1.0)


def _mesh_nodes(dim, nx, ny, nz):
    import perphil_amd.fd as fdm

    mesh = fdm.UnitCubeMesh(nx, ny, nz, hexahedral=True) if dim == 3 else fdm.UnitSquareMesh(nx, ny, quadrilateral=True)
    return mesh


def _dirichlet_sets(dim, nx, ny, nz, interior, differ):
    mesh = _mesh_nodes(dim, nx, ny, nz)
    b = np.asarray(mesh.boundary_nodes(), dtype=np.int64)
    px, py = nx + 1, ny + 1
    nodes = b
    if interior:
        # constrained nodes inside the box: in the middle of a line (a run of inner rows is cut in two), next to a line's end,
        # and a short stretch along x
        k = (nz // 2) if dim == 3 else 0
        picks = [(nx // 2, ny // 2, k), (2, ny // 2 + 1, k), (nx - 2, 2, k)] + [(nx // 3 + t, ny // 3, k) for t in range(5)]
        extra = np.array([i + px * (j + py * kk) for (i, j, kk) in picks], dtype=np.int64)
        nodes = np.unique(np.concatenate([b, extra]))
    g1, g2 = o.exact_pressures(mesh.node_coordinates(nodes), P)
    n2 = nodes[: len(nodes) // 2] if differ else nodes          # variant 4: A21 stored on its own
    return nodes, g1, n2, g2[: len(n2)]


def _export(ctx, f, rng_seed, with_solve):
    mats = [ctx.csr(w) for w in (f.MAT_A11, f.MAT_A22, f.MAT_A12, f.MAT_A21)]
    rhs, u0 = ctx.rhs()
    out = {"rhs": rhs, "u0": u0}
    for name, A in zip(("A11", "A22", "A12", "A21"), mats):
        out[name + ".indptr"], out[name + ".indices"], out[name + ".data"] = A.indptr, A.indices, A.data
    rng = np.random.default_rng(rng_seed)
    ones = np.ones(ctx.n)
    for which in (0, 1):
        out[f"dinv{which}"] = ctx.pc_apply(which, f.PC_JACOBI, ones)
        for t in range(2):
            out[f"mg{which}.{t}"] = ctx.pc_apply(which, f.PC_MG, rng.standard_normal(ctx.n), mg_smooth=1 + t)
    tm = ctx.timers()
    out["dict"] = np.array([tm["dict_operators"], tm["dict_classes"], tm["dict_status"]])
    if with_solve:
        cfg = f.SolverCfg()
        cfg.ksp_type, cfg.pc_type, cfg.restart, cfg.max_it = f.KSP_GMRES, f.PC_NONE, 30, 1000
        cfg.rtol, cfg.atol = 1e-8, 1e-12
        cfg.inner_ksp_type, cfg.inner_pc_type, cfg.inner_max_it = f.KSP_CG, f.PC_MG, 1000
        cfg.inner_rtol, cfg.inner_atol = 1e-10, 1e-300
        cfg.picard, cfg.picard_rtol, cfg.picard_atol, cfg.picard_max_it, cfg.mg_smooth = 1, 1e-8, 1e-12, 100, 1
        cfg.inner_reduction, cfg.inner_norm = 1e-1, 1
        x, info, _ = ctx.solve(cfg)
        out["x"] = x.copy()
        out["its"] = np.array([info.iterations, info.inner_iterations, info.converged])
    return out, tm


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_same_bits(A, B, tag):
    assert A.keys() == B.keys()
    for k in A:
        assert A[k].shape == B[k].shape, f"{tag}: {k}"
        bad = np.flatnonzero(_bits(A[k]) != _bits(B[k]))
        assert bad.size == 0, f"{tag}: {k} differs in {bad.size} entries, first at {bad[:5]}"


def _run(make, dim, kind, nx, ny, nz, interior, differ, uniform, dicts, poison=False, with_solve=False):
    from perphil_amd import _ffi as f

    ctx = make()
    try:
        ctx.set_option("asm_node_split_min", 1000)
        ctx.set_option("asm_uniform", uniform)
        ctx.set_option("sell_dict", dicts)
        ctx.set_option("sell_dict_min_rows", 1)
        ctx.mesh_build(dim, kind, nx, ny, nz)
        n1, g1, n2, g2 = _dirichlet_sets(dim, nx, ny, nz, interior, differ)
        ctx.set_dirichlet(0, n1, g1)
        ctx.set_dirichlet(1, n2, g2)
        if poison:
            ctx.set_option("asm_poison", 1)
        res = []
        for lines in (0, 1, 0, 2):      # (2: the line map with windows from any even row)
            ctx.set_option("asm_node_lines", lines)
            ctx.assemble(P.k1, P.k2, P.beta, P.mu, monolithic=False)
            res.append(_export(ctx, f, 11, with_solve))
        tag = f"{nx}x{ny}x{nz} interior {interior} differ {differ} uniform {uniform} dicts {dicts}"
        (e0, t0), (e1, t1), (e2, t2), (e3, t3) = res
        for k, v in e1.items():
            if v.dtype == np.float64:
                assert np.isfinite(v).all(), f"{tag}: {k} holds {np.count_nonzero(~np.isfinite(v))} non-finite entries (a row no wave stored)"
        _assert_same_bits(e0, e1, tag + " (aligned map, line map)")
        _assert_same_bits(e2, e1, tag + " (aligned map under the fused check, line map)")
        _assert_same_bits(e3, e1, tag + " (line map with even first rows, line map)")
        assert t3["asm_rows_straight"] >= t1["asm_rows_straight"]
        # the share of rows each launch stores: counted from the map; both launches together hold every row
        n = ctx.n
        assert t0["asm_rows"] == n and t1["asm_rows"] == n
        assert t0["asm_rows_straight"] == 0 and t0["asm_rows_general"] == 0          # (the aligned map is not counted)
        assert t1["asm_rows_straight"] + t1["asm_rows_general"] >= n
        if nx + 1 >= 67:
            assert t1["asm_rows_straight"] > 0
        if dicts and uniform and not interior and not differ:
            assert e1["dict"][2] == 1 and e1["dict"][0] >= 3, f"{tag}: the dictionaries were refused: {e1['dict']}"
        return t1
    finally:
        ctx.close()


HEX, QUAD = o.CELL_HEX, o.CELL_QUAD

CASES = [
    # dim kind nx ny nz interior differ uniform dicts
    (3, HEX, 32, 32, 32, 0, 0, 1, 1),      # 33 nodes per line (odd): no window fits
    (3, HEX, 33, 33, 33, 0, 0, 1, 1),      # 34 nodes per line (even)
    (3, HEX, 72, 20, 12, 0, 0, 1, 1),      # 73 per line: one window, line parity alternates
    (3, HEX, 73, 19, 11, 0, 0, 1, 1),      # 74 per line
    (3, HEX, 73, 19, 11, 0, 0, 0, 1),      # stored coordinates
    (3, HEX, 140, 12, 8, 0, 0, 1, 1),      # 141 per line: three windows, level 1 with 71 per line
    (3, HEX, 140, 12, 8, 1, 0, 1, 1),      # constrained nodes inside the box
    (3, HEX, 140, 12, 8, 1, 1, 1, 1),      # ... and different Dirichlet sets on the two fields
    (3, HEX, 140, 12, 8, 0, 1, 0, 0),      # different sets, stored coordinates, no dictionaries
    (3, HEX, 160, 10, 6, 1, 0, 0, 0),
    (3, HEX, 96, 40, 16, 0, 0, 1, 0),      # non-cubic: 97 x 41 x 17 nodes
    (2, QUAD, 70, 33, 0, 0, 0, 1, 1),
    (2, QUAD, 140, 60, 0, 1, 0, 1, 1),
    (2, QUAD, 161, 40, 0, 1, 1, 0, 0),
]


@pytest.mark.parametrize("dim,kind,nx,ny,nz,interior,differ,uniform,dicts", CASES)
def test_line_map_stores_the_bits_of_the_aligned_map(gpu_ctx_factory, dim, kind, nx, ny, nz, interior, differ, uniform, dicts):
    _run(gpu_ctx_factory, dim, kind, nx, ny, nz, interior, differ, uniform, dicts)


def test_line_map_picard_solve_is_bitwise_the_aligned_maps(gpu_ctx_factory):
    _run(gpu_ctx_factory, 3, HEX, 140, 12, 8, 1, 0, 1, 1, with_solve=True)


@pytest.mark.parametrize("dim,kind,nx,ny,nz,interior,differ", [(3, HEX, 140, 12, 8, 1, 0), (3, HEX, 73, 19, 11, 0, 1),
                                                                (2, QUAD, 140, 60, 0, 1, 0)])
def test_every_row_is_stored_by_one_of_the_two_launches(gpu_ctx_factory, dim, kind, nx, ny, nz, interior, differ):
    """Coverage: operators, right-hand side, u0 and inverse diagonals of the fine level and of every level that runs the
    node kernel start as NaNs (asm_poison); whatever the two launches of either map do not store stays NaN and fails."""
    t1 = _run(gpu_ctx_factory, dim, kind, nx, ny, nz, interior, differ, 1, 1, poison=True)
    # the line map leaves the general form the rows that need the masks - the box faces and the rows next to them (their
    # columns reach a constrained node), the 3^dim neighbours of a constrained node inside the box - plus, per line, at most
    # less than one alignment step of 8 rows at either end of the run, and a run that holds no 64 rows between such steps
    px, py, pz = nx + 1, ny + 1, (nz + 1 if dim == 3 else 1)
    lines = (py - 4) * ((pz - 4) if dim == 3 else 1)
    # (at most 8 constrained nodes inside the box here, each touching 9 lines of at most 141 nodes)
    per_line = (px - 4) - 2 * 7
    sure = per_line * lines if per_line >= 64 else 0
    assert t1["asm_rows_straight"] >= sure - (8 * 9 * 141 if interior else 0)
