"""Option sell_dict_dinv: dictionary products take the 1 / a_ii of their smoothing epilogues from the row classes' table of
inverse diagonals (SellDict::inv, pph_sell.hip) instead of streaming the dinv array.

The per-assembly check makes every row's entries those of its class bit for bit, and the table holds the assembly's own
expression (d != 0) ? 1 / d : 1 of the class's diagonal entry d, so the factor is the same double: every comparison below is
sell_dict_dinv 1 against 0 BIT FOR BIT.  With option 1 timers()["dict_dinv_products"] > 0, with option 0 it is 0.

The walk kernel (k_spmv_dict_walk) takes whole-operator products of hexahedral boxes with at least 2048 nodes per plane;
smaller boxes, tetrahedra and quadrilaterals run k_spmv_sell<DICT>.  The cases of 32^3 / 16^3 / 20 x 18 x 16 cells reach the
second, those of 48 x 48 x 16 and 64^3 cells the first (with and without class loads on the interior planes)."""
import numpy as np
import pytest

from oracle import dpp_oracle as o

from perphil_amd import _ffi as f
import perphil_amd.fd as fdm

pytestmark = pytest.mark.gpu

P = o.Params(k1=1.0, k2=0.01, beta=1.0, mu=1.0)


def _cfg():
    c = f.SolverCfg()
    c.ksp_type, c.pc_type, c.restart, c.max_it = f.KSP_GMRES, f.PC_NONE, 30, 50000
    c.rtol, c.atol = 1e-8, 1e-12
    c.inner_ksp_type, c.inner_pc_type, c.inner_max_it = f.KSP_CG, f.PC_MG, 50000
    c.inner_rtol, c.inner_atol = 1e-10, 1e-300
    c.inner_reduction, c.inner_norm = 1e-1, 1
    c.picard, c.picard_rtol, c.picard_atol, c.picard_max_it = 1, 1e-8, 1e-12, 100
    c.mg_smooth = 1           # V(1,1): the fused cycle, whose products carry the Jacobi epilogues
    return c


def _mesh(kind, nx, ny, nz):
    if kind == f.CELL_HEX:
        return fdm.UnitCubeMesh(nx, ny, nz, hexahedral=True)
    if kind == f.CELL_TET:
        return fdm.UnitCubeMesh(nx, ny, nz, hexahedral=False)
    return fdm.UnitSquareMesh(nx, ny, quadrilateral=kind == f.CELL_QUAD)


def _nodes(mesh, select):
    b = mesh.boundary_nodes()
    return b[select(mesh.node_coordinates(b))] if select else b


def _ctx(make, dinv, kind, nx, ny, nz, sel0=None, sel1=None, coefs=((P.k1, P.k2),), options=()):
    """A context with row dictionaries on every level, assembled once per coefficient pair; sel0 / sel1 pick the boundary
    nodes that carry Dirichlet data of field 0 / 1 (None: the whole boundary)."""
    ctx = make()
    ctx.set_option("sell_zwalk_min_chunks", 1)
    ctx.set_option("sell_dict", 1)
    ctx.set_option("sell_dict_min_rows", 1)
    ctx.set_option("sell_dict_dinv", dinv)
    for name, value in options:
        ctx.set_option(name, value)
    mesh = _mesh(kind, nx, ny, nz)
    ctx.mesh_build(2 if kind in (f.CELL_QUAD, f.CELL_TRI) else 3, kind, nx, ny, nz)
    for field, sel in ((0, sel0), (1, sel1)):
        b = _nodes(mesh, sel)
        g = o.exact_pressures(mesh.node_coordinates(b), P)[field]
        ctx.set_dirichlet(field, b, g)
    for k1, k2 in coefs:
        ctx.assemble(k1, k2, P.beta, P.mu, monolithic=False)
    return ctx


def _count(ctx, dinv):
    n = ctx.timers()["dict_dinv_products"]
    assert (n > 0) if dinv else (n == 0), (dinv, n)
    return n


def _applications(ctx, dinv, r):
    out = {}
    for which in (0, 1):
        for ns in (1, 2):
            out[(which, ns)] = ctx.pc_apply(which, f.PC_MG, r, mg_smooth=ns).copy()
            if ns == 1:       # (mg_smooth 2 is the general cycle: Chebyshev kernels, no Jacobi-epilogue product)
                _count(ctx, dinv)
    return out


def _solve(ctx, dinv):
    x, info, hist = ctx.solve(_cfg(), hist_cap=64)
    assert info.converged
    return x.copy(), hist.copy(), (int(info.iterations), int(info.inner_iterations)), (_count(ctx, dinv), ctx.timers()["spmv_launches"])


def _same_solve(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]


def _compare(make, kind, nx, ny, nz, sel0=None, sel1=None, coefs=((P.k1, P.k2),), solve=True, zconst=None, operators=3):
    """Applications of both cycles on a random r (and the inexact Picard solve) with sell_dict_dinv 1 and 0; returns, of the
    solve with option 1, (launches that took the table, product launches without a dot product of x)."""
    r = np.random.default_rng(3).standard_normal((nx + 1) * (ny + 1) * (nz + 1 if nz else 1))
    res = {}
    for dinv in (1, 0):
        ctx = _ctx(make, dinv, kind, nx, ny, nz, sel0, sel1, coefs)
        t = ctx.timers()
        assert t["dict_operators"] >= operators and t["dict_status"] == 1, t
        if zconst is not None:
            assert t["dict_zconst"] == zconst, t
        assert ctx.n == r.size
        res[dinv] = (_applications(ctx, dinv, r), _solve(ctx, dinv) if solve else None)
        assert ctx.timers()["dict_operators"] >= operators
        ctx.close()
    for key, z in res[1][0].items():
        np.testing.assert_array_equal(z, res[0][0][key], err_msg=str(key))
    if solve:
        _same_solve(res[1][1], res[0][1])
        return res[1][1][3]
    return None


def test_cycle_products_with_classes_constant_along_z(gpu_ctx_factory):
    """Hexahedra 32^3, data on the whole boundary (the pattern of test_row_dictionaries_inside_the_cycle): pc_apply(mg) of
    both fields, mg_smooth 1 and 2, on a random r."""
    _compare(gpu_ctx_factory, f.CELL_HEX, 32, 32, 32, solve=False, zconst=True)


def test_classes_that_change_along_z(gpu_ctx_factory):
    """16^3, data on z <= 0.5 only (the mesh of test_row_dictionary_with_classes_that_change_along_z): the same applications
    and the whole inexact Picard solve - solution, history, sweep and iteration counts."""
    low = lambda xyz: xyz[:, 2] <= 0.5
    _compare(gpu_ctx_factory, f.CELL_HEX, 16, 16, 16, low, low, zconst=False)


@pytest.mark.parametrize("nx,ny,nz", [(20, 18, 16), (48, 48, 16)])
def test_different_dirichlet_sets_per_field(gpu_ctx_factory, nx, ny, nz):
    """Field 0 with data on the whole boundary, field 1 on x = 0 and x = 1 only, then field 1 on z <= 0.5 only (A11's dictionary
    constant along z, A22's not).  With two Dirichlet sets the coupling blocks are not symmetric, are stored in full and carry
    no dictionary: their products (modes 5 / 6) read the dinv array, the cycles' products (modes 3 / 4) the tables of A11, A22
    and their levels.  The count of table launches lies strictly between the extremes - none, every product launch of the
    solve - and the solve is that of option 0 bit for bit.  (The second-dictionary path of modes 5 / 6 runs wherever both
    fields share their Dirichlet set: the classes of A12's dictionary are numbered apart from those of A11 and A22.)"""
    xfaces = lambda xyz: (xyz[:, 0] == 0.0) | (xyz[:, 0] == 1.0)
    low = lambda xyz: xyz[:, 2] <= 0.5
    # (no accessor for the class arrays: the fields are constrained on different nodes and 1 / a_ii differs on some row)
    mesh = _mesh(f.CELL_HEX, nx, ny, nz)
    assert set(_nodes(mesh, None)) != set(_nodes(mesh, xfaces))
    ctx = _ctx(gpu_ctx_factory, 1, f.CELL_HEX, nx, ny, nz, None, xfaces)
    d11, d22 = ctx.csr(f.MAT_A11).diagonal(), ctx.csr(f.MAT_A22).diagonal()
    ctx.close()
    assert np.any(1.0 / d11 != 1.0 / d22)
    for sel1 in (xfaces, low):
        table, launches = _compare(gpu_ctx_factory, f.CELL_HEX, nx, ny, nz, None, sel1, operators=2)
        assert 0 < table < launches, (table, launches)


@pytest.mark.parametrize("nx,ny,nz", [(16, 16, 16), (48, 48, 16)])
def test_reassembly_with_other_coefficients(gpu_ctx_factory, nx, ny, nz):
    """3 k2, then k2: same classes, new tables.  A table of inverse diagonals left from the first assembly would show."""
    _compare(gpu_ctx_factory, f.CELL_HEX, nx, ny, nz, coefs=((P.k1, 3.0 * P.k2), (P.k1, P.k2)))


@pytest.mark.parametrize("kind,nx,ny,nz", [(f.CELL_TET, 16, 16, 16), (f.CELL_QUAD, 40, 36, 0)])
def test_simplices_and_quadrilaterals(gpu_ctx_factory, kind, nx, ny, nz):
    """k_spmv_sell<.., DICT> with the table, through the same cycle applications."""
    _compare(gpu_ctx_factory, kind, nx, ny, nz, solve=False)


def test_walk_kernels_with_and_without_class_loads(gpu_ctx_factory):
    """48 x 48 x 16 cells (2401 nodes per plane, 17 planes): k_spmv_dict_walk<.., true> with data on the whole boundary,
    k_spmv_dict_walk<.., false> with data on z <= 0.5, and the first again with option sell_dict_zconst 0."""
    low = lambda xyz: xyz[:, 2] <= 0.5
    _compare(gpu_ctx_factory, f.CELL_HEX, 48, 48, 16, zconst=True)
    _compare(gpu_ctx_factory, f.CELL_HEX, 48, 48, 16, low, low, zconst=False)
    res = {}
    for dinv in (1, 0):
        ctx = _ctx(gpu_ctx_factory, dinv, f.CELL_HEX, 48, 48, 16, options=[("sell_dict_zconst", 0)])
        res[dinv] = _solve(ctx, dinv)
        ctx.close()
    _same_solve(res[1], res[0])


def test_refused_dictionary_falls_back_to_the_array(gpu_ctx_factory):
    """64^3 (the fused check's path), one row of A11 moved into another class on the device as in
    test_fused_dictionary_check_refuses_a_row_that_left_its_class: the next assembly refuses A11's dictionary, and this solve's
    launches for it - launched as table launches with option 1 - take the stored values and the dinv array by themselves.
    The reference is what that test compares with: the solve on the intact dictionaries (option 0), whose products are the
    stored-value products bit for bit on the same grids; the refused solve equals it with option 1 as with option 0.  (A solve
    on the plain kernels' grid sums its dot products in other groups and agrees to rounding only.)"""
    N = 64
    px = N + 1
    row = (px // 2) + px * ((px // 2) + px * (px // 2))
    ref = None
    for name, dinv in (("intact", 0), ("refused", 1), ("refused", 0)):
        ctx = _ctx(gpu_ctx_factory, dinv, f.CELL_HEX, N, N, N, coefs=((P.k1, 3.0 * P.k2), (P.k1, P.k2)),
                   options=[("sell_dict_min_rows", 100000)])
        before = ctx.timers()["dict_operators"]
        assert before >= 3
        if name == "intact":
            ref = _solve(ctx, dinv)
            ctx.close()
            continue
        ctx.set_option("sell_dict_corrupt_row", row)
        ctx.assemble(P.k1, P.k2, P.beta, P.mu, monolithic=False)            # the fused check meets the moved row
        _same_solve(_solve(ctx, dinv), ref)
        t = ctx.timers()
        assert t["dict_status"] == -2 and t["dict_operators"] == before - 1, t
        ctx.close()


def test_option_takes_0_and_1_only(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    for bad in (2, -1, 0.5):
        with pytest.raises(Exception, match="sell_dict_dinv"):
            ctx.set_option("sell_dict_dinv", bad)
    ctx.set_option("sell_dict_dinv", 0)
    ctx.set_option("sell_dict_dinv", 1)
    ctx.close()
