"""Extreme eigenvalues by Lanczos on the device (pph_extreme_eigenvalues, pph_eig.hip) through Context.extreme_eigenvalues
and the public condition-number entry points.  The reference of a device result is computed from the CSR exported from the
SAME context (dense eigvalsh up to 2 200 rows, ARPACK shift-invert / largest-algebraic above), so a failure here is the
eigen-solver's and not the assembly's; where dense algebra cannot reach, closed forms (lanczos_reference.py, pinned against
dense eigenvalues in test_lanczos_host.py).  Bars: 1e-9 relative on lambda_min and lambda_max separately - the stopping rule
guarantees 1e-10, the factor 10 covers the loss of orthogonality (observed <= 1e-12 on the CPU); 1e-12 after a breakdown,
where T is exact up to rounding (5.6e-14 observed)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lanczos_reference as lr  # noqa: E402

from oracle import dpp_oracle as o  # noqa: E402
from perphil_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu

K1, K2, BETA, MU = 1.0, 0.01, 3.0, 2.0
DENSE_ROWS = 2200
KINDS = {"quad": (2, o.CELL_QUAD), "tri": (2, o.CELL_TRI), "hex": (3, o.CELL_HEX), "tet": (3, o.CELL_TET)}
WHICH_NAME = {0: "monolithic", 2: "M", 3: "A11", 4: "A22"}


def _boundary(ctx, side_x0_only=False):
    X = ctx.coords()
    if side_x0_only:
        return np.nonzero(np.abs(X[:, 0]) < 1e-12)[0]
    return np.nonzero((np.abs(X) < 1e-12).any(axis=1) | (np.abs(X - 1.0) < 1e-12).any(axis=1))[0]


def _context(make, name, cells, degree=1, field1_x0_only=True, monolithic=True, options=(), params=(K1, K2, BETA, MU)):
    """Homogeneous data; field 0 constrained on the whole boundary, field 1 on the side x = 0 only (A12 stored in full, two
    different masks) or on the whole boundary as well."""
    dim, kind = KINDS[name]
    ctx = make()
    for k, v in options:
        ctx.set_option(k, v)
    nz = cells[2] if dim == 3 else 0
    if degree == 1:
        ctx.mesh_build(dim, kind, cells[0], cells[1], nz)
    else:
        ctx.mesh_build_lagrange(dim, kind, cells[0], cells[1], nz, degree)
    b0, b1 = _boundary(ctx), _boundary(ctx, side_x0_only=field1_x0_only)
    ctx.set_dirichlet(0, b0, np.zeros(len(b0)))
    ctx.set_dirichlet(1, b1, np.zeros(len(b1)))
    ctx.assemble(*params, monolithic=monolithic)
    return ctx


def _reference_extremes(A):
    if A.shape[0] <= DENSE_ROWS:
        ev = np.linalg.eigvalsh(A.toarray())
        return ev[0], ev[-1]
    from scipy.sparse.linalg import eigsh

    A = A.tocsc()
    lo = eigsh(A, k=1, sigma=0, which="LM", tol=0, return_eigenvectors=False)[0]
    hi = eigsh(A, k=1, which="LA", tol=0, return_eigenvectors=False)[0]
    return float(lo), float(hi)


def _assert_extremes(r, ref, what=""):
    bar = 1e-12 if r["breakdown"] else 1e-9
    print(f"{what}: steps {r['iterations']} dim {r['krylov_dimension']} breakdown {r['breakdown']} "
          f"rel. errors {abs(r['lambda_min'] / ref[0] - 1):.2e} {abs(r['lambda_max'] / ref[1] - 1):.2e} "
          f"estimates {r['estimate_min']:.1e} {r['estimate_max']:.1e} device ms {r['device_ms']:.2f}")
    assert r["converged"] == 1, (what, r)
    assert abs(r["lambda_min"] - ref[0]) <= bar * abs(ref[0]), (what, r, ref)
    assert abs(r["lambda_max"] - ref[1]) <= bar * abs(ref[1]), (what, r, ref)


# ---- 1. breakdown on tiny boxes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("name", list(KINDS))
def test_breakdown_on_tiny_boxes(gpu_ctx_factory, name, N):
    """N = 1: every node is a Dirichlet node, the operator is the identity: one step.  N = 2: one free node per field - two
    distinct eigenvalues in a block, three in the monolithic system.  The recurrence ends on an invariant subspace; the
    steps enqueued behind it divide by a beta of rounding size and are ignored."""
    ctx = _context(gpu_ctx_factory, name, (N, N, N), field1_x0_only=False)
    for which, dim_at_2 in ((0, 3), (3, 2), (4, 2)):
        A = ctx.csr(which)
        want = lr.lanczos_extremes(A)
        r = ctx.extreme_eigenvalues(which)
        assert want["breakdown"] == 1 and want["krylov_dimension"] == (1 if N == 1 else dim_at_2)
        assert r["breakdown"] == 1 and r["iterations"] == 32 and r["krylov_dimension"] == want["krylov_dimension"], r
        assert r["estimate_min"] == 0.0 and r["estimate_max"] == 0.0
        _assert_extremes(r, _reference_extremes(A), f"{name} N={N} {WHICH_NAME[which]}")


# ---- 2. all four kinds at degree 1 ------------------------------------------------------------------------------------
DEG1 = {"quad": (16, 15), "tri": (13, 11), "hex": (7, 5, 6), "tet": (5, 4, 3)}


@pytest.mark.parametrize("name", list(DEG1))
def test_all_cell_kinds_at_degree_1(gpu_ctx_factory, name):
    ctx = _context(gpu_ctx_factory, name, DEG1[name])
    for which in (0, 2, 3, 4):
        A = ctx.csr(which)
        assert abs(A - A.T).max() <= 1e-14 * abs(A).max()
        _assert_extremes(ctx.extreme_eigenvalues(which), _reference_extremes(A), f"{name} {WHICH_NAME[which]}")


# ---- 3. degree 2: CSR products ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cells", [("quad", (6, 5)), ("tet", (3, 3, 2))])
def test_degree_2_contexts(gpu_ctx_factory, name, cells):
    ctx = _context(gpu_ctx_factory, name, cells, degree=2)
    for which in (0, 3, 4):
        _assert_extremes(ctx.extreme_eigenvalues(which), _reference_extremes(ctx.csr(which)), f"{name} deg 2 {WHICH_NAME[which]}")


# ---- 4. the reference's goldens through the public API ----------------------------------------------------------------
_COLS = (("monolithic", "cond_monolithic"), ("macro", "cond_macro"), ("micro", "cond_micro"))


def test_G3_on_the_device(gpu_ctx_factory, goldens):
    """The 10 x 10 notebook values through estimate_condition_numbers(on_device=True) and, form by form, through
    conditioning.condition_number_on_device; equal to the host path's results."""
    import perphil_amd as pa
    from perphil_amd import conditioning, fd, iterative_bench as ib

    mesh = pa.create_mesh(10, 10, quadrilateral=True)
    _, V = pa.create_function_spaces(mesh)
    W = V * V
    params = pa.DPPParameters(k1=1.0, k2=1 / 1e2, beta=1.0, mu=1)
    _, p1e, _, p2e = pa.exact_expressions(mesh, params)
    bcs = [fd.DirichletBC(W.sub(0), p1e, "on_boundary"), fd.DirichletBC(W.sub(1), p2e, "on_boundary")]
    g = goldens["G3_condition_numbers_10x10"]
    dev = ib.estimate_condition_numbers(W, params=params, bcs=bcs, on_device=True)
    host = ib.estimate_condition_numbers(W, params=params, bcs=bcs, use_sparse=True, num_of_factors=0)
    for k in ("monolithic", "macro", "micro"):
        assert dev[k] == pytest.approx(g[k], rel=1e-9) and dev[k] == pytest.approx(host[k], rel=1e-9), (k, dev, host)
    a, _ = pa.dpp_form(W, params)
    (am, _), (ai, _) = pa.dpp_delayed_form(V, V, params, fd.Function(V), fd.Function(V))
    assert conditioning.condition_number_on_device(a, bcs) == pytest.approx(g["monolithic"], rel=1e-9)
    assert conditioning.condition_number_on_device(am, [bcs[0]]) == pytest.approx(g["macro"], rel=1e-9)
    assert conditioning.condition_number_on_device(ai, [bcs[1]]) == pytest.approx(g["micro"], rel=1e-9)
    assert conditioning.condition_number_on_device(a, bcs, zero_tol=10.0) == float("inf")   # lambda_min <= zero_tol


@pytest.mark.parametrize("N", [16, 32, 64])
def test_G4_rows_on_the_device(gpu_ctx_factory, goldens, N):
    """conditioning.csv rows N = 16, 32 and 64 (8 450 dofs: the row no dense SVD in a test reaches)."""
    from perphil_amd import iterative_bench as ib

    g = next(r for r in goldens["G4_conditioning_2d"] if int(r["N"]) == N)
    _, _, W = ib.build_spaces(ib.build_mesh(N, N))
    dev = ib.estimate_condition_numbers(W, on_device=True)
    for k, col in _COLS:
        assert dev[k] == pytest.approx(g[col], rel=1e-9), (k, dev[k], g[col])
    if N <= 16:
        host = ib.estimate_condition_numbers(W, use_sparse=True, num_of_factors=0)
        for k, _ in _COLS:
            assert dev[k] == pytest.approx(host[k], rel=1e-9), (k, dev, host)


@pytest.mark.parametrize("N", [8, 14, 16])
def test_G5_rows_on_the_device(gpu_ctx_factory, goldens, N):
    """conditioning_3d.csv rows N = 8, 14 and 16 (6 750 and 9 826 dofs: minutes of host SVD, pinned by no other test)."""
    import perphil_amd as pa
    from perphil_amd import fd
    from perphil_amd.iterative_bench import estimate_condition_numbers
    from perphil_amd.manufactured_solutions import exact_expressions_3d

    g = next(r for r in goldens["G5_conditioning_3d_hex"] if int(r["N"]) == N)
    mesh = fd.UnitCubeMesh(N, N, N, hexahedral=True)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    params = pa.DPPParameters(k1=1.0, k2=1.0 / 1e2, beta=1.0, mu=1.0)
    _u1, p1e, _u2, p2e = exact_expressions_3d(mesh, params)
    bcs = [fd.DirichletBC(W.sub(0), p1e, "on_boundary"), fd.DirichletBC(W.sub(1), p2e, "on_boundary")]
    assert W.dim() == int(g["n_dofs"])
    dev = estimate_condition_numbers(W, params=params, bcs=bcs, on_device=True)
    for k, col in _COLS:
        assert dev[k] == pytest.approx(g[col], rel=1e-9), (k, dev[k], g[col])
    if N <= 8:
        host = estimate_condition_numbers(W, params=params, bcs=bcs, use_sparse=True, num_of_factors=0)
        for k, _ in _COLS:
            assert dev[k] == pytest.approx(host[k], rel=1e-9), (k, dev, host)


# ---- 5. closed forms at a size dense algebra cannot reach -------------------------------------------------------------
def test_closed_forms_on_hex_33x32x31(gpu_ctx_factory):
    cells = (33, 32, 31)
    ctx = _context(gpu_ctx_factory, "hex", cells, field1_x0_only=False, monolithic=False)
    assert ctx.n == 34 * 33 * 32 and ctx.n < lr.GRID_CAPACITY_ROWS
    _assert_extremes(ctx.extreme_eigenvalues(3), lr.box_block_extremes(cells, K1 / MU, BETA / MU), "hex 33x32x31 A11")
    _assert_extremes(ctx.extreme_eigenvalues(4), lr.box_block_extremes(cells, K2 / MU, BETA / MU), "hex 33x32x31 A22")
    _assert_extremes(ctx.extreme_eigenvalues(2), lr.box_mass_extremes(cells), "hex 33x32x31 M")


# ---- 6. past the grid capacity of the new kernels ---------------------------------------------------------------------
def test_rows_past_the_grid_capacity(gpu_ctx_factory):
    """k_lanczos_update / k_lanczos_scale run min(ceil(pairs / 256), 1024) blocks of 256 threads on pairs of rows: with more
    than 1024 x 256 x 2 = 524 288 rows a thread takes a second pair (hex 80^3: 531 441 nodes, an odd count: the single last
    row as well).  kappa(M) tends to 64 (the cube of the 1D ratio 4): 288 steps in the NumPy restatement."""
    N = 80
    ctx = gpu_ctx_factory()
    ctx.mesh_build(3, o.CELL_HEX, N, N, N)
    assert ctx.n == 81 ** 3 and ctx.n > lr.GRID_CAPACITY_ROWS and ctx.n % 2 == 1
    r = ctx.extreme_eigenvalues(2)
    _assert_extremes(r, lr.box_mass_extremes((N, N, N)), "hex 80^3 M")


# ---- 7. product paths agree bit for bit -------------------------------------------------------------------------------
def test_product_paths_agree(gpu_ctx_factory):
    """hex 32^3, A11: the stored stencil-ELL values and the row-dictionary walk give bitwise equal products, so the whole
    iteration is the same; the CSR product agrees to the bar; a second call on a context repeats the first bit for bit."""
    sets = {"plain": (("sell_dict", 0),),
            "dict": (("sell_dict", 1), ("sell_dict_min_rows", 1), ("sell_zwalk_min_chunks", 1)),
            "csr": (("op_format", 0),)}
    keys = ("lambda_min", "lambda_max", "iterations", "estimate_min", "estimate_max", "krylov_dimension", "breakdown")
    res = {}
    for name, opts in sets.items():
        ctx = _context(gpu_ctx_factory, "hex", (32, 32, 32), field1_x0_only=False, monolithic=False, options=opts)
        assert (ctx.timers()["dict_operators"] >= 1) == (name == "dict"), (name, ctx.timers())
        r1, r2 = ctx.extreme_eigenvalues(3), ctx.extreme_eigenvalues(3)
        assert r1["converged"] == 1
        assert [r1[k] for k in keys] == [r2[k] for k in keys], (name, r1, r2)
        res[name] = r1
        ctx.close()
    assert [res["plain"][k] for k in keys] == [res["dict"][k] for k in keys], res
    for k in ("lambda_min", "lambda_max"):
        assert res["csr"][k] == pytest.approx(res["plain"][k], rel=1e-9)
    _assert_extremes(res["plain"], lr.box_block_extremes((32, 32, 32), K1 / MU, BETA / MU), "hex 32^3 A11")


# ---- 8. Ritz vectors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cells", [("quad", (16, 15)), ("hex", (7, 5, 6))])
def test_ritz_vectors(gpu_ctx_factory, name, cells):
    ctx = _context(gpu_ctx_factory, name, cells)
    A = ctx.csr(0)
    ref = _reference_extremes(A)
    plain = ctx.extreme_eigenvalues(0)
    r = ctx.extreme_eigenvalues(0, vectors=True)
    assert (r["lambda_min"], r["lambda_max"], r["iterations"]) == (plain["lambda_min"], plain["lambda_max"], plain["iterations"])
    for end, lam in (("min", ref[0]), ("max", ref[1])):
        y = r[f"vector_{end}"].cpu().numpy()
        rq, res = r[f"rayleigh_{end}"], r[f"residual_{end}"]
        print(f"{name} {end}: |rq / lambda - 1| {abs(rq / lam - 1):.2e}  residual / lambda_max {res / ref[1]:.2e}")
        assert y.shape == (A.shape[0],) and abs(np.linalg.norm(y) - 1.0) <= 1e-13
        assert abs(rq - lam) <= 1e-10 * abs(lam), (end, rq, lam)
        assert abs(res - np.linalg.norm(A @ y - rq * y)) <= 1e-12 * ref[1], (end, res)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx_factory):
    ctx = _context(gpu_ctx_factory, "hex", (7, 5, 6), monolithic=False)
    for which in (1, 5, 6, 7):
        with pytest.raises(ValueError):
            ctx.extreme_eigenvalues(which)
    with pytest.raises(ValueError, match="monolithic"):
        ctx.extreme_eigenvalues(0)
    r = ctx.extreme_eigenvalues(3, max_it=8)
    assert r["converged"] == 0 and r["iterations"] == 8 and r["breakdown"] == 0
    assert np.isfinite([r["lambda_min"], r["lambda_max"], r["estimate_min"], r["estimate_max"]]).all()
    ref = _reference_extremes(ctx.csr(3))
    assert ref[0] <= r["lambda_min"] * (1 + 1e-12) and r["lambda_max"] <= ref[1] * (1 + 1e-12)   # Ritz values lie inside the spectrum


def test_unconverged_run_raises_through_the_public_api(gpu_ctx_factory, monkeypatch):
    import perphil_amd as pa
    from perphil_amd import conditioning, fd

    mesh = fd.UnitCubeMesh(7, 5, 6, hexahedral=True)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    params = pa.DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
    a, _ = pa.dpp_form(W, params)
    bcs = [fd.DirichletBC(W.sub(0), fd.Constant(0.0), "on_boundary"), fd.DirichletBC(W.sub(1), fd.Constant(0.0), "on_boundary")]
    assert np.isfinite(conditioning.condition_number_on_device(a, bcs))
    real = _ffi.Context.extreme_eigenvalues
    monkeypatch.setattr(_ffi.Context, "extreme_eigenvalues", lambda self, which, tol=1e-10: real(self, which, tol=tol, max_it=8))
    with pytest.raises(RuntimeError, match="did not converge"):
        conditioning.condition_number_on_device(a, bcs)
