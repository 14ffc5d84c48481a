"""Option l3_order: fine-level kernels start their sweep where the kernel before them stopped, so that the vectors both touch
are met in the Infinity Cache.  The order-free elementwise and transfer kernels run their grid-stride loops descending
(PPH_DIR_LOOP, pph_internal.h), the walk products (k_spmv_dict_walk) take their ranges through an order - reversed, and with
l3_walk_order 1 plane-band major.  No item's arithmetic, no range and no partial-sum slot changes, so every comparison below
is l3_order 1 against 0 BIT FOR BIT.  With option 1 timers()["l3_order_descending"] > 0, with option 0 it is 0.

Every context has row dictionaries on all levels (sell_dict_min_rows 1, sell_zwalk_min_chunks 1) and l3_order_min_rows 0, so
that these small shapes take the new order.  The walk kernel takes hexahedral boxes with at least 2048 nodes per plane
(48 x 48 x 16, 52 x 50 x 9, 52 x 50 x 8, 104 x 104 x 100); on 16^3 and 32^3 the elementwise and transfer kernels alone carry
the order."""
import numpy as np
import pytest

from oracle import dpp_oracle as o

from perphil_amd import _ffi as f
import perphil_amd.fd as fdm

pytestmark = pytest.mark.gpu

P = o.Params(k1=1.0, k2=0.01, beta=1.0, mu=1.0)


def LOW(xyz):
    return xyz[:, 2] <= 0.5


def _cfg():
    c = f.SolverCfg()
    c.ksp_type, c.pc_type, c.restart, c.max_it = f.KSP_GMRES, f.PC_NONE, 30, 50000
    c.rtol, c.atol = 1e-8, 1e-12
    c.inner_ksp_type, c.inner_pc_type, c.inner_max_it = f.KSP_CG, f.PC_MG, 50000
    c.inner_rtol, c.inner_atol = 1e-10, 1e-300
    c.inner_reduction, c.inner_norm = 1e-1, 1
    c.picard, c.picard_rtol, c.picard_atol, c.picard_max_it = 1, 1e-8, 1e-12, 100
    c.mg_smooth = 1           # V(1,1): the fused cycle
    return c


def _ctx(make, l3, nx, ny, nz, sel=None, options=()):
    """A context on nx x ny x nz hexahedra with dictionaries on every level and the option on every vector; sel picks the
    boundary nodes that carry Dirichlet data (None: the whole boundary)."""
    ctx = make()
    ctx.set_option("sell_zwalk_min_chunks", 1)
    ctx.set_option("sell_dict", 1)
    ctx.set_option("sell_dict_min_rows", 1)
    ctx.set_option("l3_order_min_rows", 0)
    ctx.set_option("l3_order", l3)
    for name, value in options:
        ctx.set_option(name, value)
    mesh = fdm.UnitCubeMesh(nx, ny, nz, hexahedral=True)
    ctx.mesh_build(3, f.CELL_HEX, nx, ny, nz)
    b = mesh.boundary_nodes()
    if sel is not None:
        b = b[sel(mesh.node_coordinates(b))]
    g = o.exact_pressures(mesh.node_coordinates(b), P)
    for field in (0, 1):
        ctx.set_dirichlet(field, b, g[field])
    ctx.assemble(P.k1, P.k2, P.beta, P.mu, monolithic=False)
    return ctx


def _count(ctx, l3):
    n = ctx.timers()["l3_order_descending"]
    assert (n > 0) if l3 else (n == 0), (l3, n)
    return n


def _applications(ctx, l3, r):
    out = {}
    for which in (0, 1):
        out[which] = ctx.pc_apply(which, f.PC_MG, r, mg_smooth=1).copy()
        _count(ctx, l3)
    return out


def _solve(ctx, l3):
    x, info, hist = ctx.solve(_cfg(), hist_cap=64)
    assert info.converged
    _count(ctx, l3)
    return x.copy(), hist.copy(), (int(info.iterations), int(info.inner_iterations)), float(info.resnorm)


def _same_solve(a, b, msg=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=msg)
    np.testing.assert_array_equal(a[1], b[1], err_msg=msg)
    assert a[2] == b[2], msg
    assert a[3] == b[3], msg


def _run(make, l3, nx, ny, nz, sel, options, solve, zconst):
    r = np.random.default_rng(3).standard_normal((nx + 1) * (ny + 1) * (nz + 1))
    ctx = _ctx(make, l3, nx, ny, nz, sel, options)
    t = ctx.timers()
    assert t["dict_operators"] >= 3 and t["dict_status"] == 1, t
    if zconst is not None:
        assert t["dict_zconst"] == zconst, t
    assert ctx.n == r.size
    res = (_applications(ctx, l3, r), _solve(ctx, l3) if solve else None)
    ctx.close()
    return res


_REF = {}


def _reference(make, nx, ny, nz, sel, options, solve, zconst):
    """The results with l3_order 0, computed once per (shape, data, grid options) and shared by the orders compared with it."""
    key = (nx, ny, nz, sel is not None, tuple(options), solve)
    if key not in _REF:
        _REF[key] = _run(make, 0, nx, ny, nz, sel, options, solve, zconst)
    return _REF[key]


def _compare(make, nx, ny, nz, sel=None, options=(), solve=True, zconst=None, walk_orders=(0, 1)):
    """pc_apply(mg) of both fields with mg_smooth 1 on a random r (and the inexact Picard solve: solution, history, sweep and
    iteration counts, resnorm) with l3_order 1 - once per order of the walk's ranges - against l3_order 0."""
    ref = _reference(make, nx, ny, nz, sel, options, solve, zconst)
    for wo in walk_orders:
        got = _run(make, 1, nx, ny, nz, sel, tuple(options) + (("l3_walk_order", wo),), solve, zconst)
        for which, z in got[0].items():
            np.testing.assert_array_equal(z, ref[0][which], err_msg=f"field {which}, l3_walk_order {wo}")
        if solve:
            _same_solve(got[1], ref[1], f"l3_walk_order {wo}")


@pytest.mark.parametrize("blocks", [8, 13, None])
def test_walk_products_on_constant_classes(gpu_ctx_factory, blocks):
    """48 x 48 x 16 cells, data on the whole boundary: the smallest shape the walk kernel takes (49^2 = 2401 >= 2048 nodes per
    plane; 5 in-plane chunks x 17 planes = 85 steps), classes constant along z.  sell_dict_blocks 8 and 13: ranges that straddle
    columns and do not divide the 85 steps evenly; the default grid: one step per range."""
    options = () if blocks is None else (("sell_dict_blocks", blocks),)
    _compare(gpu_ctx_factory, 48, 48, 16, options=options, zconst=True)


def test_elementwise_and_transfer_kernels_alone(gpu_ctx_factory):
    """16^3, data on z <= 0.5 only: classes change along z, 289 nodes per plane - no walk kernel; the elementwise and transfer
    kernels alone carry the order."""
    _compare(gpu_ctx_factory, 16, 16, 16, LOW, zconst=False, walk_orders=(1,))


def test_walk_products_with_class_loads(gpu_ctx_factory):
    """48 x 48 x 16 with data on z <= 0.5: the walk kernel without constant classes."""
    _compare(gpu_ctx_factory, 48, 48, 16, LOW, zconst=False)


@pytest.mark.parametrize("nz", [9, 8])
def test_odd_line_length_and_short_ranges(gpu_ctx_factory, nz):
    """52 x 50 x 9: 53 nodes per grid line (the pair kernels' last pair of a line has one node), 10 planes - ranges shorter than
    the walk kernel's straight-line loop.  9 cells along z cannot be halved, so that mesh has one level (Chebyshev steps
    around a walk product, no transfers); 52 x 50 x 8 has two, and its interpolation runs the single-node tail."""
    _compare(gpu_ctx_factory, 52, 50, nz)


def test_more_than_one_grid_stride_trip(gpu_ctx_factory):
    """104 x 104 x 100 (1 113 525 nodes): more than one trip of the grid-stride loops, whose grids end at 2048 workgroups of 256
    threads (x 2 rows for the elementwise kernels) - the descending loop starts in a partly filled last trip.  Applications only."""
    n = 105 * 105 * 101
    assert 2048 * 256 * 2 < n
    _compare(gpu_ctx_factory, 104, 104, 100, solve=False)


def test_replayed_graph_equals_the_eager_body(gpu_ctx_factory):
    """32^3, use_graphs 2: the iteration bodies are captured and replayed.  A body starts from a fixed direction, so a replay
    equals its capture - and the eager loop with the option on, and the eager loop with the option off."""
    res = {}
    for name, l3, graphs in (("off", 0, 0), ("eager", 1, 0), ("replayed", 1, 2)):
        ctx = _ctx(gpu_ctx_factory, l3, 32, 32, 32, options=(("use_graphs", graphs),))
        res[name] = _solve(ctx, l3)
        ctx.close()
    _same_solve(res["replayed"], res["eager"], "replayed against eager")
    _same_solve(res["eager"], res["off"], "l3_order 1 against 0")


def test_options_take_0_and_1_only(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    for name in ("l3_order", "l3_walk_order"):
        for bad in (2, -1, 0.5):
            with pytest.raises(Exception, match=name):
                ctx.set_option(name, bad)
        ctx.set_option(name, 0)
        ctx.set_option(name, 1)
    ctx.close()
