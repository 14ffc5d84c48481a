"""Extreme eigenvalues of preconditioned operators on the device (pph_preconditioned_extremes, pph_eig.hip) through
Context.preconditioned_extremes and the public entry points of perphil_amd.conditioning.

References are dense and built from the SAME context: A = ctx.csr(which) restricted to the free rows, A_ff = C C^T, and the
eigenvalues of C^T B_ff C with B_ff built column by column through ctx.pc_apply (ILU(0) and the multigrid cycles of the
blocks), from the CSR itself (Jacobi, 2 x 2 block-Jacobi) or from the oracle's ILU(0) of the exported monolithic CSR (there
is no pc_apply of the monolithic system).  A failure is then the eigen-solver's, not the assembly's or the cycle's.

Bars (tests/README_pclanczos.md): 1e-9 relative per end at tol 1e-10 for the linear preconditioners - the project's Lanczos
bar: the stopping rule guarantees 1e-10, the factor 10 covers the loss of orthogonality; 1e-12 after a breakdown, where T is
exact up to rounding; for the multigrid cycles at the default tol 1e-4 the Ritz residual bound of the end plus the distance
2a between the cycle and its symmetric part plus the project's bar."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pclanczos_reference as pr  # noqa: E402

from oracle import dpp_oracle as o  # noqa: E402
from perphil_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu

K1, K2, BETA, MU = 1.0, 0.01, 3.0, 2.0
KINDS = {"quad": (2, o.CELL_QUAD), "tri": (2, o.CELL_TRI), "hex": (3, o.CELL_HEX), "tet": (3, o.CELL_TET)}
WHICH_NAME = {0: "monolithic", 2: "M", 3: "A11", 4: "A22"}
PC_NAME = {_ffi.PC_JACOBI: "jacobi", _ffi.PC_BLOCK2: "pph_block2", _ffi.PC_ILU: "ilu", _ffi.PC_MG: "mg", _ffi.PC_PMG: "pph_pmg"}


def _boundary(ctx, side_x0_only=False):
    X = ctx.coords()
    if side_x0_only:
        return np.nonzero(np.abs(X[:, 0]) < 1e-12)[0]
    return np.nonzero((np.abs(X) < 1e-12).any(axis=1) | (np.abs(X - 1.0) < 1e-12).any(axis=1))[0]


def _context(make, name, cells, degree=1, field1_x0_only=True, monolithic=True, options=()):
    """test_lanczos_gpu.py's contexts: homogeneous data; field 0 constrained on the whole boundary, field 1 on the side
    x = 0 only (two different masks) or on the whole boundary as well.  Returns (context, the two masks)."""
    dim, kind = KINDS[name]
    ctx = make()
    for k, v in options:
        ctx.set_option(k, v)
    nz = cells[2] if dim == 3 else 0
    if degree == 1:
        ctx.mesh_build(dim, kind, cells[0], cells[1], nz)
    else:
        ctx.mesh_build_lagrange(dim, kind, cells[0], cells[1], nz, degree)
    masks = []
    for f, b in enumerate((_boundary(ctx), _boundary(ctx, side_x0_only=field1_x0_only))):
        ctx.set_dirichlet(f, b, np.zeros(len(b)))
        m = np.zeros(ctx.n, dtype=bool)
        m[b] = True
        masks.append(m)
    ctx.assemble(K1, K2, BETA, MU, monolithic=monolithic)
    return ctx, masks


def _reference(ctx, masks, which, pc, mg_smooth=2):
    """Dense spectrum of B A on the free rows, from the context's own operator and preconditioner."""
    n = ctx.n
    A = ctx.csr(which)
    mask = np.concatenate(masks) if which == 0 else masks[which - 3]
    free = np.nonzero(~mask)[0]
    if pc == _ffi.PC_JACOBI:
        Bff = np.diag(1.0 / A.diagonal()[free])
    elif pc == _ffi.PC_BLOCK2:
        i = np.arange(n)
        d11, d22 = A.diagonal()[:n], A.diagonal()[n:]
        d12, d21 = np.asarray(A[i, n + i]).ravel(), np.asarray(A[n + i, i]).ravel()
        det = d11 * d22 - d12 * d21
        B = np.zeros((2 * n, 2 * n))
        B[i, i], B[i, n + i], B[n + i, i], B[n + i, n + i] = d22 / det, -d12 / det, -d21 / det, d11 / det
        Bff = B[np.ix_(free, free)]
    elif which == 0:
        assert pc == _ffi.PC_ILU
        LU = o.ilu0(A).toarray()   # the pattern of the export, explicit zeros kept: the device's
        L, U = np.tril(LU, -1) + np.eye(2 * n), np.triu(LU)
        Bff = np.linalg.solve(U, np.linalg.solve(L, np.eye(2 * n)))[np.ix_(free, free)]
    else:
        Bff = pr.dense_operator(lambda e: ctx.pc_apply(which - 3, pc, e, mg_smooth=mg_smooth), n, free)
    return pr.dense_pencil(A, Bff, free)


def _assert_extremes(r, ref, what):
    bar = 1e-12 if r["breakdown"] else 1e-9
    errs = [abs(r["lambda_min"] / ref["lambda_min"] - 1), abs(r["lambda_max"] / ref["lambda_max"] - 1)]
    print(f"{what}: steps {r['iterations']} dim {r['krylov_dimension']} breakdown {r['breakdown']} lambda "
          f"{r['lambda_min']:.6g} {r['lambda_max']:.6g} kappa {r['kappa']:.6g} rel. errors {errs[0]:.2e} {errs[1]:.2e} "
          f"estimates {r['estimate_min']:.1e} {r['estimate_max']:.1e} a {ref.get('a', 0.0):.1e} device ms {r['device_ms']:.2f}")
    assert r["converged"] == 1, (what, r)
    assert errs[0] <= bar and errs[1] <= bar, (what, r, ref["lambda_min"], ref["lambda_max"])
    assert r["kappa"] == r["lambda_max"] / r["lambda_min"]


def _assert_multigrid(r, ref, what):
    """Item 3's rule: conditions on the run and on the reference, then the Ritz residual bound of each end plus the
    symmetrisation 2a plus the project's bar, and Ritz values inside the spectrum."""
    a, lo, hi = ref["a"], ref["lambda_min"], ref["lambda_max"]
    print(f"{what}: steps {r['iterations']} lambda {r['lambda_min']:.9f} {r['lambda_max']:.9f} (dense {lo:.9f} {hi:.9f}) "
          f"errors {abs(r['lambda_min'] - lo):.2e} {abs(r['lambda_max'] - hi):.2e} estimates {r['estimate_min']:.1e} "
          f"{r['estimate_max']:.1e} a {a:.2e} kappa {r['kappa']:.6f} device ms {r['device_ms']:.2f} setup ms {r['setup_ms']:.2f}")
    assert r["converged"] == 1 and r["breakdown"] == 0, (what, r)
    assert r["estimate_min"] <= 1e-4 * abs(r["lambda_min"]) and r["estimate_max"] <= 1e-4 * abs(r["lambda_max"]), (what, r)
    assert a <= 1e-6 * lo, (what, a, lo)
    assert abs(r["lambda_min"] - lo) <= r["estimate_min"] + 2 * a + 1e-9 * abs(lo), (what, r, lo)
    assert abs(r["lambda_max"] - hi) <= r["estimate_max"] + 2 * a + 1e-9 * abs(hi), (what, r, hi)
    assert lo * (1 - 1e-9) - 2 * a <= r["lambda_min"] and r["lambda_max"] <= hi * (1 + 1e-9) + 2 * a, (what, r, lo, hi)


# ---- 1. tiny boxes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(KINDS))
def test_breakdown_on_tiny_boxes(gpu_ctx_factory, name):
    """N = 2: one free node per field - D^-1 A has one eigenvalue on a block (1: the recurrence ends at once), two on the
    monolithic system.  The steps enqueued behind the breakdown divide by a beta of rounding size and are ignored."""
    ctx, masks = _context(gpu_ctx_factory, name, (2, 2, 2), field1_x0_only=False)
    for which, dim in ((3, 1), (4, 1), (0, 2)):
        r = ctx.preconditioned_extremes(which, _ffi.PC_JACOBI)
        assert r["breakdown"] == 1 and r["iterations"] == 16 and r["krylov_dimension"] == dim, r
        assert r["estimate_min"] == 0.0 and r["estimate_max"] == 0.0
        _assert_extremes(r, _reference(ctx, masks, which, _ffi.PC_JACOBI), f"{name} N=2 {WHICH_NAME[which]} jacobi")


@pytest.mark.parametrize("name", list(KINDS))
def test_no_free_rows(gpu_ctx_factory, name):
    """N = 1: every node is a Dirichlet node."""
    ctx, _ = _context(gpu_ctx_factory, name, (1, 1, 1), field1_x0_only=False)
    for which in (0, 3, 4):
        with pytest.raises(ValueError, match="no free rows"):
            ctx.preconditioned_extremes(which, _ffi.PC_JACOBI)


# ---- 2. linear preconditioners at degree 1 ----------------------------------------------------------------------------
DEG1 = {"quad": (16, 15), "tri": (13, 11), "hex": (7, 5, 6), "tet": (5, 4, 3)}   # test_lanczos_gpu.py's set
LINEAR_CASES = [(3, _ffi.PC_JACOBI), (3, _ffi.PC_ILU), (4, _ffi.PC_JACOBI), (4, _ffi.PC_ILU), (0, _ffi.PC_JACOBI),
                (0, _ffi.PC_BLOCK2), (0, _ffi.PC_ILU), (2, _ffi.PC_JACOBI)]


@pytest.mark.parametrize("name", list(DEG1))
def test_linear_preconditioners_at_degree_1(gpu_ctx_factory, name):
    ctx, masks = _context(gpu_ctx_factory, name, DEG1[name])
    # (272, 168, 336 and 120 rows: all even - the odd last row is taken by the multigrid meshes below and by hex 80^3)
    for which, pc in LINEAR_CASES:
        r = ctx.preconditioned_extremes(which, pc, tol=1e-10)
        if which == 2:   # no constrained rows: all of D^-1 M
            M = ctx.csr(2)
            s = 1.0 / np.sqrt(M.diagonal())
            ev = np.linalg.eigvalsh(M.toarray() * s[:, None] * s[None, :])
            ref = {"lambda_min": ev[0], "lambda_max": ev[-1]}
        else:
            ref = _reference(ctx, masks, which, pc)
        _assert_extremes(r, ref, f"{name} {WHICH_NAME[which]} {PC_NAME[pc]}")


# ---- 3. multigrid at the defaults -------------------------------------------------------------------------------------
MG_MESHES = {"quad": (16, 12), "tri": (12, 8), "hex": (8, 4, 6), "tet": (4, 4, 4)}   # coarsenable, odd node counts


@pytest.mark.parametrize("name", list(MG_MESHES))
def test_multigrid_at_the_defaults(gpu_ctx_factory, name):
    ctx, masks = _context(gpu_ctx_factory, name, MG_MESHES[name], monolithic=False)
    assert ctx.n % 2 == 1 and ctx.n == {"quad": 221, "tri": 117, "hex": 315, "tet": 125}[name]
    for which in (3, 4):
        r = ctx.preconditioned_extremes(which, _ffi.PC_MG)
        _assert_multigrid(r, _reference(ctx, masks, which, _ffi.PC_MG), f"{name} {WHICH_NAME[which]} mg")
        assert ctx.preconditioned_extremes(which, _ffi.PC_PMG)["lambda_min"] == r["lambda_min"]   # at degree 1 pph_pmg is mg
        assert ctx.preconditioned_extremes(which, _ffi.PC_MG)["setup_ms"] == 0.0                  # the hierarchy is up to date


# ---- 4. degree 2 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cells", [("quad", (6, 5)), ("tet", (3, 3, 2))])
def test_degree_2_linear_preconditioners(gpu_ctx_factory, name, cells):
    ctx, masks = _context(gpu_ctx_factory, name, cells, degree=2)
    for which, pc in ((3, _ffi.PC_JACOBI), (3, _ffi.PC_ILU), (4, _ffi.PC_JACOBI), (4, _ffi.PC_ILU), (0, _ffi.PC_JACOBI),
                      (0, _ffi.PC_BLOCK2)):
        r = ctx.preconditioned_extremes(which, pc, tol=1e-10)
        _assert_extremes(r, _reference(ctx, masks, which, pc), f"{name} deg 2 {WHICH_NAME[which]} {PC_NAME[pc]}")


def test_degree_2_p_multigrid(gpu_ctx_factory):
    ctx, masks = _context(gpu_ctx_factory, "quad", (8, 4), degree=2, monolithic=False)
    for which in (3, 4):
        r = ctx.preconditioned_extremes(which, _ffi.PC_PMG)
        _assert_multigrid(r, _reference(ctx, masks, which, _ffi.PC_PMG), f"quad 8x4 deg 2 {WHICH_NAME[which]} pph_pmg")
    with pytest.raises(ValueError, match="pph_pmg"):
        ctx.preconditioned_extremes(3, _ffi.PC_MG)


# ---- 5. past the grid capacity of the new kernels ---------------------------------------------------------------------
def test_rows_past_the_grid_capacity(gpu_ctx_factory):
    """k_pclanczos_update / k_pclanczos_scale run min(ceil(pairs / 256), 1024) blocks of 256 threads on pairs of rows: with
    more than 1024 x 256 x 2 = 524 288 rows a thread takes a second pair (hex 80^3: 531 441 nodes, an odd count: the single
    last row as well).  D^-1 M has the extremes (1/8, 27/8) on any box of hexes (kappa 27): 1216 steps in the NumPy
    restatement at tol 1e-10 (the lower end, where the eigenvalues of the 1D pencils pile up at 1/2, is the slow one)."""
    N = 80
    ctx = gpu_ctx_factory()
    ctx.mesh_build(3, o.CELL_HEX, N, N, N)
    assert ctx.n == 81 ** 3 and ctx.n > pr.GRID_CAPACITY_ROWS and ctx.n % 2 == 1
    r = ctx.preconditioned_extremes(2, _ffi.PC_JACOBI, tol=1e-10)
    _assert_extremes(r, {"lambda_min": 0.125, "lambda_max": 3.375}, "hex 80^3 M jacobi")


# ---- 6. product paths and determinism ---------------------------------------------------------------------------------
def test_product_paths_agree(gpu_ctx_factory):
    """hex 32^3, A11 under Jacobi: the stored stencil-ELL values and the row-dictionary walk give bitwise equal products, the
    dots and the vector kernels have one grid and one order whatever the product - the whole iteration is the same; a second
    call on a context repeats the first bit for bit."""
    sets = {"plain": (("sell_dict", 0),),
            "dict": (("sell_dict", 1), ("sell_dict_min_rows", 1), ("sell_zwalk_min_chunks", 1))}
    keys = ("lambda_min", "lambda_max", "iterations", "estimate_min", "estimate_max", "krylov_dimension", "breakdown", "kappa")
    res = {}
    for name, opts in sets.items():
        ctx, _ = _context(gpu_ctx_factory, "hex", (32, 32, 32), field1_x0_only=False, monolithic=False, options=opts)
        assert (ctx.timers()["dict_operators"] >= 1) == (name == "dict"), (name, ctx.timers())
        r1 = ctx.preconditioned_extremes(3, _ffi.PC_JACOBI, tol=1e-10)
        r2 = ctx.preconditioned_extremes(3, _ffi.PC_JACOBI, tol=1e-10)
        assert r1["converged"] == 1
        assert [r1[k] for k in keys] == [r2[k] for k in keys], (name, r1, r2)
        res[name] = r1
        ctx.close()
    assert [res["plain"][k] for k in keys] == [res["dict"][k] for k in keys], res
    print("hex 32^3 A11 jacobi:", res["plain"])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx_factory):
    ctx, masks = _context(gpu_ctx_factory, "hex", (7, 5, 6), monolithic=False)
    for which, pc in ((3, _ffi.PC_FIELDSPLIT), (3, _ffi.PC_NONE), (0, _ffi.PC_MG), (2, _ffi.PC_MG), (1, _ffi.PC_JACOBI),
                      (5, _ffi.PC_JACOBI), (6, _ffi.PC_JACOBI), (3, _ffi.PC_BLOCK2), (2, _ffi.PC_ILU)):
        with pytest.raises(ValueError):
            ctx.preconditioned_extremes(which, pc)
    with pytest.raises(ValueError, match="pph_extreme_eigenvalues"):
        ctx.preconditioned_extremes(3, _ffi.PC_NONE)
    with pytest.raises(ValueError, match="not a symmetric"):
        ctx.preconditioned_extremes(3, _ffi.PC_FIELDSPLIT)
    with pytest.raises(ValueError, match="monolithic"):
        ctx.preconditioned_extremes(0, _ffi.PC_JACOBI)
    r = ctx.preconditioned_extremes(3, _ffi.PC_JACOBI, max_it=8)
    assert r["converged"] == 0 and r["iterations"] == 8 and r["breakdown"] == 0
    assert np.isfinite([r["lambda_min"], r["lambda_max"], r["estimate_min"], r["estimate_max"], r["kappa"]]).all()
    ref = _reference(ctx, masks, 3, _ffi.PC_JACOBI)
    assert ref["lambda_min"] <= r["lambda_min"] * (1 + 1e-12) and r["lambda_max"] <= ref["lambda_max"] * (1 + 1e-12)   # Ritz values lie inside the spectrum


# ---- 8. public API on the G3 mesh -------------------------------------------------------------------------------------
def test_public_api_on_the_G3_mesh(gpu_ctx_factory):
    import perphil_amd as pa
    from perphil_amd import conditioning, fd
    from perphil_amd import solver_parameters as sp

    mesh = pa.create_mesh(10, 10, quadrilateral=True)
    _, V = pa.create_function_spaces(mesh)
    W = V * V
    params = pa.DPPParameters(k1=1.0, k2=1 / 1e2, beta=1.0, mu=1)
    _, p1e, _, p2e = pa.exact_expressions(mesh, params)
    bcs = [fd.DirichletBC(W.sub(0), p1e, "on_boundary"), fd.DirichletBC(W.sub(1), p2e, "on_boundary")]
    a, _ = pa.dpp_form(W, params)
    (am, _), (ai, _) = pa.dpp_delayed_form(V, V, params, fd.Function(V), fd.Function(V))

    def dense_kappa(form, b):
        A = conditioning.get_matrix_data_from_form(form, b).sparse_csr_data.toarray()
        free = np.nonzero((np.abs(A - np.diag(np.diag(A))).sum(axis=1) > 0) | (np.diag(A) != 1.0))[0]   # not a unit row
        Af = A[np.ix_(free, free)]
        s = 1.0 / np.sqrt(np.diag(Af))
        ev = np.linalg.eigvalsh(Af * s[:, None] * s[None, :])
        return ev[-1] / ev[0]

    want = {}
    for name, form, b in (("monolithic", a, bcs), ("macro", am, [bcs[0]]), ("micro", ai, [bcs[1]])):
        want[name] = dense_kappa(form, b)
        got = conditioning.preconditioned_condition_number(form, b, "jacobi", tol=1e-10)
        print(f"G3 mesh {name} jacobi: kappa {got:.9g} dense {want[name]:.9g} rel. error {abs(got / want[name] - 1):.2e}")
        assert got == pytest.approx(want[name], rel=1e-9)
    opts = {"ksp_type": "cg", "pc_type": "jacobi"}
    eff = conditioning.effective_condition_numbers(W, params, bcs, opts, tol=1e-10)
    assert set(eff) == {"monolithic"} and eff["monolithic"] == pytest.approx(want["monolithic"], rel=1e-9)
    assert eff["monolithic"] == conditioning.preconditioned_condition_number(a, bcs, "jacobi", tol=1e-10)
    eff = conditioning.effective_condition_numbers(W, params, bcs, sp.PICARD_MG_SOLVER_PARAMS, nonlinear=True)
    print("G3 mesh, PICARD_MG_SOLVER_PARAMS:", eff)
    assert set(eff) == {"macro", "micro"} and 1.0 < eff["macro"] < 2.0 and 1.0 < eff["micro"] < 2.0


def test_unconverged_run_raises_through_the_public_api(gpu_ctx_factory, monkeypatch):
    import perphil_amd as pa
    from perphil_amd import conditioning, fd

    mesh = fd.UnitCubeMesh(7, 5, 6, hexahedral=True)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    a, _ = pa.dpp_form(W, pa.DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0))
    bcs = [fd.DirichletBC(W.sub(0), fd.Constant(0.0), "on_boundary"), fd.DirichletBC(W.sub(1), fd.Constant(0.0), "on_boundary")]
    assert np.isfinite(conditioning.preconditioned_condition_number(a, bcs, "pph_block2"))
    real = _ffi.Context.preconditioned_extremes
    monkeypatch.setattr(_ffi.Context, "preconditioned_extremes",
                        lambda self, which, pc, mg_smooth=2, tol=1e-4: real(self, which, pc, mg_smooth=mg_smooth, tol=tol, max_it=8))
    with pytest.raises(RuntimeError, match="did not converge"):
        conditioning.preconditioned_condition_number(a, bcs, "pph_block2", tol=1e-10)
