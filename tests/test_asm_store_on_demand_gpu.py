"""Operator values on demand (option asm_store_values, default 0): an assembly whose straight-line rows are checked against
the row dictionaries inside the node kernel does not store them - the products run on the dictionaries and never read them.
The stored values are a fallback, written when somebody asks: a reader that is not a dictionary product (sell_values_ensure),
or - when a check refuses a dictionary on the device - the guarded launch behind the level's last check kernel.

The reference in every test is the same sequence of calls on a context with asm_store_values 1 (every assembly stores every
entry); every comparison is bitwise."""
import numpy as np
import pytest

from oracle import dpp_oracle as o

P = o.Params(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
# three assemblies: the first builds the dictionaries, the second has other coefficients, the third the final ones
COEFS = [(P.k1, 3.0 * P.k2), (2.0 * P.k1, P.k2), (P.k1, P.k2)]
SMALL = {"asm_node_split_min": 1, "sell_dict_min_rows": 1, "sell_zwalk_min_chunks": 1}
# `windows`: the fine level's wave map holds straight-line windows (64 consecutive interior rows of ONE grid line: lines of
# at least 73 nodes - a line of 65 has 63 interior rows).  The first four shapes are the ones the change was specified with;
# on the three hexahedral ones the straight-line launch is empty (asm_rows_straight == 0 on the parent commit as well), so they
# pin the bookkeeping and the general launch only, and each has a sibling with longer lines that runs the new kernels.
SHAPES = {
    # the two-launch fused check at the default thresholds (274 625 / 389 017 rows per block)
    "hex64": dict(dim=3, cells=(64, 64, 64), opts={"sell_dict_min_rows": 100000}, bc="all", windows=False),
    "hex72": dict(dim=3, cells=(72, 72, 72), opts={"sell_dict_min_rows": 100000}, bc="all", windows=True),
    # pxy >= 2048, pz = 13 >= 8: the walk kernel with constant classes
    "hex48x44x12": dict(dim=3, cells=(48, 44, 12), opts=SMALL, bc="all", windows=False),
    "hex80x28x12": dict(dim=3, cells=(80, 28, 12), opts=SMALL, bc="all", windows=True),
    # 2D: k_spmv_sell<DICT>
    "quad96x80": dict(dim=2, cells=(96, 80, 0), opts=SMALL, bc="all", windows=True),
    # Dirichlet data on the lower half of the boundary only: the classes change along z
    "hex16_lower_half": dict(dim=3, cells=(16, 16, 16), opts=SMALL, bc="lower", windows=False),
    "hex72x16x16_lower_half": dict(dim=3, cells=(72, 16, 16), opts=SMALL, bc="lower", windows=True),
    # level 1 (73 x 9 x 9 = 5913 rows, above the multigrid tail) has dictionaries and windows too: the level operators' variant
    "hex144x16x16_two_levels": dict(dim=3, cells=(144, 16, 16), opts=SMALL, bc="all", windows=True),
}
ALL = list(SHAPES)


def _ffi():
    from perphil_amd import _ffi

    return _ffi


def _cfg():
    """bench.py's Picard configuration"""
    f = _ffi()
    c = f.SolverCfg()
    c.ksp_type, c.pc_type, c.restart, c.max_it = f.KSP_GMRES, f.PC_FIELDSPLIT, 30, 50000
    c.rtol, c.atol = 1e-8, 1e-12
    c.inner_ksp_type, c.inner_pc_type, c.inner_max_it = f.KSP_CG, f.PC_MG, 50000
    c.inner_rtol, c.inner_atol = 1e-10, 1e-300
    c.picard, c.picard_rtol, c.picard_atol, c.picard_max_it = 1, 1e-8, 1e-12, 100
    c.mg_smooth = 1
    c.inner_reduction = 1e-1
    c.inner_norm = 1
    return c


def _boundary(shape, which=None):
    """(nodes, g1, g2) of the shape's Dirichlet set (node i + px (j + py k) at (i / nx, j / ny, k / nz))"""
    dim = shape["dim"]
    nx, ny, nz = shape["cells"]
    px, py, pz = nx + 1, ny + 1, (nz + 1 if dim == 3 else 1)
    k, j, i = np.meshgrid(np.arange(pz), np.arange(py), np.arange(px), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    on = (i == 0) | (i == nx) | (j == 0) | (j == ny)
    if dim == 3:
        on |= (k == 0) | (k == nz)
    which = which or shape["bc"]
    if which == "lower":
        on &= (2 * k <= nz)
    elif which == "x0":
        on &= (i == 0)
    nodes = np.flatnonzero(on).astype(np.int64)
    coords = np.stack([i[nodes] / nx, j[nodes] / ny] + ([k[nodes] / nz] if dim == 3 else []), axis=1)
    g1, g2 = o.exact_pressures(coords, P)
    return nodes, g1, g2


def _mats():
    f = _ffi()
    return (f.MAT_A11, f.MAT_A22, f.MAT_A12)


def _open(make, name, store, poison=0):
    f = _ffi()
    shape = SHAPES[name]
    ctx = make()
    ctx.set_option("asm_store_values", store)
    for k, v in shape["opts"].items():
        ctx.set_option(k, v)
    ctx.set_option("asm_poison", poison)
    nx, ny, nz = shape["cells"]
    ctx.mesh_build(shape["dim"], f.CELL_HEX if shape["dim"] == 3 else f.CELL_QUAD, nx, ny, nz)
    b, g1, g2 = _boundary(shape)
    ctx.set_dirichlet(0, b, g1)
    ctx.set_dirichlet(1, b, g2)
    return ctx


def _assemble(ctx, count=3):
    for k1, k2 in COEFS[3 - count:]:
        ctx.assemble(k1, k2, P.beta, P.mu, monolithic=False)


def _products(ctx):
    x = np.random.default_rng(7).standard_normal(ctx.n)
    return [ctx.spmv(m, x) for m in _mats()]


def _solve(ctx):
    x, info, hist = ctx.solve(_cfg(), hist_cap=32)
    assert info.converged
    return x.copy(), hist.copy(), (info.iterations, info.inner_iterations)


def _counters(ctx):
    t = ctx.timers()
    return (t["asm_values_stale"], t["asm_values_materialized"], t["asm_store_repairs"])


_REF = {}


def _reference(name):
    """The sequence of the tests on a context that stores everything (asm_store_values 1): computed once per shape."""
    if name in _REF:
        return _REF[name]
    f = _ffi()
    made = []

    def make():
        made.append(f.Context(0))
        return made[-1]

    r = {"counters": []}
    ctx = _open(make, name, 1)
    _assemble(ctx)
    r["counters"].append(_counters(ctx))
    r["dict_operators"] = ctx.timers()["dict_operators"]
    r["products"] = _products(ctx)
    r["x"], r["hist"], r["its"] = _solve(ctx)
    r["dict_operators_solved"] = ctx.timers()["dict_operators"]     # (with the multigrid levels' dictionaries)
    r["counters"].append(_counters(ctx))
    r["csr"] = [ctx.csr(m).data.copy() for m in _mats()]
    r["counters"].append(_counters(ctx))
    ctx.set_option("sell_dict", 0)
    r["products_plain"] = _products(ctx)
    r["counters"].append(_counters(ctx))
    ctx.close()
    # another Dirichlet set for field 0 with nothing assembled after it, then with a new assembly
    ctx = _open(make, name, 1)
    _assemble(ctx)
    r["after_bc"] = _input_change(ctx, name)
    r["counters"].append(_counters(ctx))
    ctx.close()
    assert np.isfinite(r["x"]).all() and all(np.isfinite(p).all() for p in r["products"])
    _REF[name] = r
    return r


def _input_change(ctx, name):
    b, g1, _ = _boundary(SHAPES[name], "x0")
    ctx.set_dirichlet(0, b, g1)
    ctx.set_option("sell_dict", 0)
    x = np.random.default_rng(7).standard_normal(ctx.n)
    try:
        first = ctx.spmv(_ffi().MAT_A11, x)
    except (RuntimeError, ValueError) as e:      # (a changed Dirichlet set drops the assembled system: the product is refused until the next assembly)
        first = str(e)
    ctx.assemble(P.k1, P.k2, P.beta, P.mu, monolithic=False)
    return first, ctx.spmv(_ffi().MAT_A11, x)


def _assert_same(got, ref):
    if isinstance(ref, str) or isinstance(got, str):
        assert got == ref
    else:
        np.testing.assert_array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_products_and_solve_equal_the_storing_assembly(gpu_ctx_factory, name):
    """1. Three assemblies, the products of A11 / A22 / A12 and the benchmark's Picard solve: bitwise the storing context's,
    with the fine level's straight-line rows never stored."""
    ref = _reference(name)
    ctx = _open(gpu_ctx_factory, name, 0)
    _assemble(ctx)
    t = ctx.timers()
    assert t["asm_values_stale"] == 1 and (t["asm_rows_straight"] > 0) == SHAPES[name]["windows"], t
    assert t["dict_operators"] == ref["dict_operators"] >= 3, t
    for got, want in zip(_products(ctx), ref["products"]):
        np.testing.assert_array_equal(got, want)
    x, hist, its = _solve(ctx)
    np.testing.assert_array_equal(x, ref["x"])
    np.testing.assert_array_equal(hist, ref["hist"])
    assert its == ref["its"]
    assert _counters(ctx) == (1, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_nobody_reads_what_was_not_stored(gpu_ctx_factory, name):
    """2. asm_poison fills the outputs with NaNs ahead of every assembly: the rows the check-mode launch does not store stay NaN
    (seen through an export that takes the arrays as they are), yet products and solve are the reference's and finite."""
    ref = _reference(name)
    ctx = _open(gpu_ctx_factory, name, 0, poison=1)
    _assemble(ctx)
    for got, want in zip(_products(ctx), ref["products"]):
        np.testing.assert_array_equal(got, want)
    x, hist, its = _solve(ctx)
    assert np.isfinite(x).all()
    np.testing.assert_array_equal(x, ref["x"])
    np.testing.assert_array_equal(hist, ref["hist"])
    assert its == ref["its"]
    assert _counters(ctx) == (1, 0, 0)
    ctx.set_option("asm_values_peek", 1)
    raw = ctx.csr(_ffi().MAT_A11).data
    nan = np.isnan(raw)
    assert nan.any() == SHAPES[name]["windows"] and not nan.all()
    np.testing.assert_array_equal(raw[~nan], ref["csr"][0][~nan])      # (the general launch's rows are stored as ever)
    assert _counters(ctx) == (1, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_export_materialises_once(gpu_ctx_factory, name):
    """3. After the poisoned sequence the CSR exports equal the reference's entry for entry: one launch wrote the missing
    rows, a second export launches nothing."""
    ref = _reference(name)
    ctx = _open(gpu_ctx_factory, name, 0, poison=1)
    _assemble(ctx)
    _solve(ctx)
    assert _counters(ctx) == (1, 0, 0)
    for m, want in zip(_mats(), ref["csr"]):
        np.testing.assert_array_equal(ctx.csr(m).data, want)
    assert _counters(ctx) == (0, 1, 0)
    np.testing.assert_array_equal(ctx.csr(_mats()[0]).data, ref["csr"][0])
    assert _counters(ctx) == (0, 1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_dictionaries_switched_off_without_an_assembly(gpu_ctx_factory, name):
    """3b. sell_dict 0 takes effect at once: the first plain product writes the missing rows first."""
    ref = _reference(name)
    ctx = _open(gpu_ctx_factory, name, 0, poison=1)
    _assemble(ctx)
    ctx.set_option("sell_dict", 0)
    assert _counters(ctx) == (1, 0, 0)
    for got, want in zip(_products(ctx), ref["products_plain"]):
        np.testing.assert_array_equal(got, want)
    assert _counters(ctx) == (0, 1, 0)


def _refusal(ctx, name, which):
    """two assemblies, a row of A11 moved into another class on the device, the final assembly, two solves"""
    _assemble(ctx, 2)
    px = SHAPES[name]["cells"][0] + 1
    row = (px // 2) + px * ((px // 2) + px * (px // 2)) if which == "interior" else 1 + px * ((px // 2) + px * (px // 2))
    ctx.set_option("sell_dict_corrupt_row", row)
    _assemble(ctx, 1)
    stale = _counters(ctx)[0]
    first = _solve(ctx)
    t = ctx.timers()
    return first, _solve(ctx), t, stale            # (the second solve: A11 on the plain kernels)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["interior", "near_boundary"])
@pytest.mark.parametrize("name", ["hex64", "hex72"])
def test_refusal_on_the_device_is_repaired_on_the_device(gpu_ctx_factory, name, which):
    """4. A row moved into another class on the device (an interior row: found by the straight-line launch's compare where the
    row lies in a window; a row next to the boundary: by the read-back of the general rows): the products already enqueued fall
    back to the stored values, which the guarded launch behind the last check kernel has written by then.  Reference: the same
    calls on a storing context; its first solve is also the solve of the untouched dictionaries, bit for bit.  (The second solve
    runs A11 on the plain kernels, whose grids - and so the order of the partial sums of the dot products - are not the
    dictionary kernels': it equals the storing context's second solve, not its first.)"""
    ref = _reference(name)
    key = (name, which)
    if key not in _REF:
        rctx = _open(gpu_ctx_factory, name, 1, poison=1)
        _REF[key] = _refusal(rctx, name, which)
        assert _counters(rctx) == (0, 0, 0) and _REF[key][3] == 0
    want1, want2, tr, _ = _REF[key]
    ctx = _open(gpu_ctx_factory, name, 0, poison=1)
    (x, hist, its), (x2, hist2, its2), t, stale = _refusal(ctx, name, which)
    assert stale == 1
    assert np.isfinite(x).all() and np.isfinite(hist).all() and np.isfinite(x2).all() and np.isfinite(hist2).all()
    np.testing.assert_array_equal(x, ref["x"])
    np.testing.assert_array_equal(hist, ref["hist"])
    np.testing.assert_array_equal(x, want1[0])
    np.testing.assert_array_equal(hist, want1[1])
    assert its == want1[2] == ref["its"]
    assert t["dict_status"] == -2 == tr["dict_status"] and t["dict_operators"] == tr["dict_operators"], (t, tr)
    assert t["asm_store_repairs"] >= 1 and t["asm_values_stale"] == 0 and t["asm_values_materialized"] == 0, t
    np.testing.assert_array_equal(x2, want2[0])
    np.testing.assert_array_equal(hist2, want2[1])
    assert its2 == want2[2]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["hex48x44x12", "hex80x28x12", "quad96x80"])
def test_dictionaries_poisoned_behind_the_hosts_back(gpu_ctx_factory, name, mode):
    """5. sell_dict_poison marks the fine blocks' dictionaries as refused on the device only - no repair launch will run, so
    the option writes the missing rows before it poisons."""
    ref = _reference(name)
    ctx = _open(gpu_ctx_factory, name, 0, poison=1)
    _assemble(ctx)
    ctx.set_option("sell_dict_poison", mode)
    assert _counters(ctx) == (0, 1, 0)
    for got, want in zip(_products(ctx), ref["products"]):
        np.testing.assert_array_equal(got, want)
    x, hist, its = _solve(ctx)
    np.testing.assert_array_equal(x, ref["x"])
    np.testing.assert_array_equal(hist, ref["hist"])
    t = ctx.timers()
    if mode == 2:
        assert t["dict_status"] == -2 and t["dict_operators"] == ref["dict_operators_solved"] - 3, t
    assert _counters(ctx) == (0, 1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hex48x44x12", "hex80x28x12", "quad96x80"])
def test_dirichlet_set_changed_while_values_are_stale(gpu_ctx_factory, name):
    """6. Another node set for field 0 after an on-demand assembly, then sell_dict 0 and a product of A11: what the storing
    context does - before and after the next assembly.  The missing rows were written before the masks changed."""
    ref = _reference(name)
    ctx = _open(gpu_ctx_factory, name, 0, poison=1)
    _assemble(ctx)
    assert _counters(ctx) == (1, 0, 0)
    first, second = _input_change(ctx, name)
    _assert_same(first, ref["after_bc"][0])
    _assert_same(second, ref["after_bc"][1])
    assert _counters(ctx) == (0, 1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_storing_assembly_reports_nothing_stale(name):
    """7. asm_store_values 1: nothing stale, nothing written on demand, nothing repaired - at every point of the sequence."""
    assert _reference(name)["counters"] == [(0, 0, 0)] * 5
