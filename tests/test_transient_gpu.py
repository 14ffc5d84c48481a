"""The step right-hand side of the transient DPP model on the device (pph_dpp_step_rhs*, perphil_amd/csrc/pph_transient.hip)
through Context.step_rhs, against the restatement of tests/transient_reference.py.

b = -F A_unel p for a random mixed field p.  Bar: |b_i - ref_i| <= 1e3 eps (|A_unel| |p|)_i - the rounding bound of a sum of
at most about 200 terms (27 neighbours x 2 fields x up to 8 boxes folded into a coefficient first), each term bounded by its
entry of |A_unel| |p|, with a decade and more of slack; a wrong box matrix, a skipped or a phantom box shows at 1e-2 of the
row's scale.  Entries on constrained dofs are exactly 0, and two calls give the same bits.

Shapes: all four cell kinds with unequal nx, ny, nz (an axis mix-up shows), 1 x 1 (x 1) (every node is a corner: every box
test is taken), 1025 x 513 nodes (more than one pass of the kernel's grid: transient_reference.step_kernel_loops), the CSR
formulation at degree 1 (option asm_uniform 0: stored coordinates) and on a degree-2 mesh.
Every test prints its worst figure before it asserts.

The second half of the file: the shifted assembly (pph_assemble_dpp_shifted) against the restatement through every assembly
option, one application of every preconditioner on a shifted system against restated cycles, the step loop
(pph_transient_begin / pph_transient_steps) against the closed form and direct stepping on nine solver families, the balance
identity, the refusals, and solve_dpp_transient end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import dpp_oracle as o  # noqa: E402
from perphil_amd import _ffi  # noqa: E402
import cmg_reference as CR  # noqa: E402
import transient_reference as T  # noqa: E402

pytestmark = pytest.mark.gpu

CF = T.Coefs(1.3, 0.02, 3.0, 2.0)
BAR = 1e3 * T.EPS
SMALL = [(o.CELL_QUAD, 5, 3, 0), (o.CELL_TRI, 4, 3, 0), (o.CELL_HEX, 5, 3, 4), (o.CELL_TET, 3, 4, 2),
         (o.CELL_QUAD, 1, 1, 0), (o.CELL_TRI, 1, 2, 0), (o.CELL_HEX, 1, 1, 1), (o.CELL_TET, 2, 1, 1)]
NAMES = ("quad", "tri", "hex", "tet")


def _id(c):
    return f"{NAMES[c[0]]}{c[1]}x{c[2]}x{c[3]}"


def _dim(kind):
    return 2 if kind in (o.CELL_QUAD, o.CELL_TRI) else 3


def _dirichlet_sets(kind, nx, ny, nz, which):
    """'none', 'shared' (both fields on the whole boundary) or 'mixed' (cmg_reference.mixed_nodes: field 1 on two sides plus
    interior nodes)."""
    om = o.build_mesh(_dim(kind), kind, nx, ny, nz)
    if which == "none":
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if which == "shared":
        b = o.boundary_nodes(om)
        return b, b
    return CR.mixed_nodes(kind, nx, ny, nz)


def _context(make, kind, nx, ny, nz, nodes, degree=1, options=()):
    ctx = make()
    for name, v in options:
        ctx.set_option(name, v)
    if degree == 1:
        ctx.mesh_build(_dim(kind), kind, nx, ny, nz)
    else:
        ctx.mesh_build_lagrange(_dim(kind), kind, nx, ny, nz, degree)
    rng = np.random.default_rng(5)
    for f in (0, 1):
        ctx.set_dirichlet(f, nodes[f], rng.standard_normal(len(nodes[f])))   # (the values must not enter b)
    return ctx


def _check(tag, b, ref, bound, con):
    ratio = float((abs(b - ref) / np.maximum(bound, 1e-300)).max() / T.EPS)
    print(f"{tag}: worst |diff| / (eps |A||p|) = {ratio:.2f} (bar 1e3), {int(con.sum())} constrained dofs")
    assert np.all(abs(b - ref) <= BAR * bound)
    assert np.all(b[con] == 0.0) and not np.any(np.signbit(b[con]))


@pytest.mark.parametrize("sets", ["none", "shared", "mixed"])
@pytest.mark.parametrize("case", SMALL, ids=_id)
def test_step_rhs_matches_the_restatement(gpu_ctx_factory, case, sets):
    kind, nx, ny, nz = case
    if sets == "mixed" and min(nx, ny) < 2:
        sets = "shared"   # (no interior node to pick; the shared sets are run under the other id as well)
    om, K, M = T.scalar_matrices(_dim(kind), kind, nx, ny, nz)
    n = om.num_nodes
    nodes = _dirichlet_sets(kind, nx, ny, nz, sets)
    masks = T.masks_of(n, *nodes)
    con = np.concatenate(masks)
    p = np.random.default_rng(100 + SMALL.index(case)).standard_normal(2 * n) * 10.0 ** np.random.default_rng(7).uniform(-2, 2, 2 * n)
    ref, bound = T.step_rhs(K, M, CF, masks, p), T.abs_bound(K, M, CF, p)
    ctx = _context(gpu_ctx_factory, kind, nx, ny, nz, nodes)
    assert ctx.n == n
    b = ctx.step_rhs(p, CF.k1, CF.k2, CF.beta, CF.mu)
    _check(f"{_id(case)} {sets}", b, ref, bound, con)
    # two calls, and the device-tensor variant: the same bits
    assert np.array_equal(b, ctx.step_rhs(p, CF.k1, CF.k2, CF.beta, CF.mu))
    pd = torch.from_numpy(p.copy()).cuda()
    bd = ctx.step_rhs(pd, CF.k1, CF.k2, CF.beta, CF.mu)
    assert bd.is_cuda and np.array_equal(bd.cpu().numpy(), b) and np.array_equal(pd.cpu().numpy(), p)
    # -F dpp_nodal_flux(p): the stored-CSR formulation of the same quantity
    r = -ctx.dpp_nodal_flux(p, CF.k1, CF.k2, CF.beta, CF.mu)
    r[con] = 0.0
    assert np.all(abs(b - r) <= BAR * bound)


def _device_reference(ctx, masks, p):
    """Reference and bound from the context's own exported K and M (meshes too large for the oracle's Python assembly)."""
    K, M = ctx.csr(_ffi.MAT_K), ctx.csr(_ffi.MAT_M)
    return T.step_rhs(K, M, CF, masks, p), T.abs_bound(K, M, CF, p)


def test_more_nodes_than_one_pass_of_the_grid(gpu_ctx_factory):
    """1024 x 512 quadrilaterals: 525 825 nodes, the 2048 workgroups cover 524 288 per pass.  Powers of two, because the
    reference here is the context's exported K, integrated on the STORED coordinates i / n: their rounding (one eps of a
    coordinate of magnitude 1 against an edge of 1 / n) enters K at n eps relative - the reference's own error, which on
    800 x 700 cells uses up the bar (measured: 948 eps of |A| |p|) while the kernel's closed form carries none of it.  With
    n a power of two the stored coordinates are exact and the comparison is about the kernel again."""
    kind, nx, ny = o.CELL_QUAD, 1024, 512
    n = (nx + 1) * (ny + 1)
    assert T.step_kernel_loops(n)
    idx = np.arange(n)
    i, j = idx % (nx + 1), idx // (nx + 1)
    b0 = idx[(i == 0) | (i == nx) | (j == 0) | (j == ny)]
    b1 = idx[(i == 0) | (j == ny) | ((i == 400) & (j == ny - 1)) | (idx == n - 2)]   # (constrained dofs in the second pass too)
    masks = T.masks_of(n, b0, b1)
    p = np.random.default_rng(11).standard_normal(2 * n)
    ctx = _context(gpu_ctx_factory, kind, nx, ny, 0, (b0, b1))
    b = ctx.step_rhs(p, CF.k1, CF.k2, CF.beta, CF.mu)
    ref, bound = _device_reference(ctx, masks, p)
    _check("quad1024x512", b, ref, bound, np.concatenate(masks))
    assert np.array_equal(b, ctx.step_rhs(p, CF.k1, CF.k2, CF.beta, CF.mu))
    assert np.count_nonzero(ref[2048 * 256:n]) > 400   # (the rows of the second pass are not trivially right)


@pytest.mark.parametrize("case,degree,options", [((o.CELL_HEX, 5, 3, 4), 1, (("asm_uniform", 0),)), ((o.CELL_QUAD, 5, 3, 0), 2, ()),
                                                 ((o.CELL_TET, 3, 2, 3), 2, ())],
                         ids=["hex5x3x4-stored-coordinates", "quad5x3-deg2", "tet3x2x3-deg2"])
def test_csr_formulation(gpu_ctx_factory, case, degree, options):
    """Where the kernel's closed forms do not apply the entry point walks the stored K and M: the bits of
    -F pph_dpp_nodal_flux(p)."""
    kind, nx, ny, nz = case
    ctx = _context(gpu_ctx_factory, kind, nx, ny, nz, (np.zeros(0, dtype=np.int64),) * 2, degree, options)
    n = ctx.n
    rng = np.random.default_rng(21)
    nodes = (np.sort(rng.choice(n, n // 3, replace=False)), np.sort(rng.choice(n, n // 4, replace=False)))
    for f in (0, 1):
        ctx.set_dirichlet(f, nodes[f], np.ones(len(nodes[f])))
    masks = T.masks_of(n, *nodes)
    con = np.concatenate(masks)
    p = rng.standard_normal(2 * n)
    b = ctx.step_rhs(p, CF.k1, CF.k2, CF.beta, CF.mu)
    ref, bound = _device_reference(ctx, masks, p)
    _check(f"{_id(case)} degree {degree}", b, ref, bound, con)
    r = -ctx.dpp_nodal_flux(p, CF.k1, CF.k2, CF.beta, CF.mu)
    r[con] = 0.0
    assert np.array_equal(b, r)
    assert np.array_equal(b, ctx.step_rhs(p, CF.k1, CF.k2, CF.beta, CF.mu))
    if degree == 1:   # ... and the matrix-free kernel agrees with it on the same context
        ctx.set_option("asm_uniform", 1)
        _check(f"{_id(case)} matrix-free after the option", ctx.step_rhs(p, CF.k1, CF.k2, CF.beta, CF.mu), ref, bound, con)


def test_refusals_leave_the_context_usable(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    p = np.ones(8)
    out = np.empty(8)

    def call(fn, a, b, mu=1.0):
        return fn(ctx._h, 1.0, 1.0, 1.0, mu, a, b)

    ptr = p.ctypes.data_as(C.c_void_p)
    optr = out.ctypes.data_as(C.c_void_p)
    assert call(_ffi.lib.pph_dpp_step_rhs, ptr, optr) == _ffi.PPH_ERR_INVALID
    assert b"before pph_mesh_build" in _ffi.lib.pph_last_error(ctx._h)
    ctx.mesh_build(2, o.CELL_QUAD, 1, 1)
    d = torch.ones(8, dtype=torch.float64, device="cuda")
    dptr = C.c_void_p(d.data_ptr())
    for fn, a, b, mu, msg in [(_ffi.lib.pph_dpp_step_rhs, None, optr, 1.0, b"NULL buffer"),
                              (_ffi.lib.pph_dpp_step_rhs, ptr, None, 1.0, b"NULL buffer"),
                              (_ffi.lib.pph_dpp_step_rhs, ptr, ptr, 1.0, b"different buffers"),
                              (_ffi.lib.pph_dpp_step_rhs, ptr, optr, 0.0, b"mu must not be 0"),
                              (_ffi.lib.pph_dpp_step_rhs_device, dptr, dptr, 1.0, b"different buffers"),
                              (_ffi.lib.pph_dpp_step_rhs_device, None, dptr, 1.0, b"NULL buffer"),
                              (_ffi.lib.pph_dpp_step_rhs_device, dptr, None, 1.0, b"NULL buffer")]:
        assert call(fn, a, b, mu) == _ffi.PPH_ERR_INVALID
        assert msg in _ffi.lib.pph_last_error(ctx._h), _ffi.lib.pph_last_error(ctx._h)
    with pytest.raises(ValueError):
        ctx.step_rhs(np.ones(7), 1.0, 1.0, 1.0, 1.0)
    # the context still works: constants are in the kernel of K, so b = -(beta/mu) M (p1 - p2) = 0 for p1 = p2
    b = ctx.step_rhs(p, 1.0, 0.5, 2.0, 1.0)
    assert abs(b).max() <= 1e-15
    q = np.concatenate([np.ones(4), np.zeros(4)])
    b = ctx.step_rhs(q, 1.0, 0.5, 2.0, 1.0)   # M 1 = 1/4 per corner of the unit square
    assert np.allclose(b, np.concatenate([-0.5 * np.ones(4), 0.5 * np.ones(4)]), rtol=0, atol=1e-15)


# ======================================================================================================================
# shifted assembly (pph_assemble_dpp_shifted), the step loop (pph_transient_begin / pph_transient_steps) and its refusals
# ======================================================================================================================
from perphil_amd import solver, solver_parameters as spar  # noqa: E402

SIGMA = (7.5, 120.0)
VAL_TOL = 1e-12          # tests/test_gpu_parity.py: blocks and right-hand side against the oracle, relative to the largest entry
SHIFT_CASES = [(o.CELL_QUAD, 5, 3, 0), (o.CELL_TRI, 4, 3, 0), (o.CELL_HEX, 3, 4, 2), (o.CELL_TET, 3, 2, 3)]
# Device solutions against the restatement's direct (splu) stepping, relative to max |p|, all solves to rtol 1e-12.
# Measured worst value over the cases of this file: see STEP_MEASURED; the bar is ten times that - a decade for the drift of
# iterative solves over the steps; a wrong coefficient shows at 1e-2 or worse.
STEP_MEASURED = 8.53e-13
STEP_TOL = 10 * STEP_MEASURED


def _cfg(params, nonlinear=False):
    cfg, info = solver.translate_options(params, nonlinear=nonlinear)
    cfg.rtol, cfg.atol = 1e-12, 1e-300
    cfg.inner_rtol, cfg.inner_atol = 1e-13, 1e-300
    cfg.picard_rtol, cfg.picard_atol = 1e-12, 1e-300
    cfg.inner_reduction = 0.0
    return cfg


def _dirichlet_data(n, nodes, seed):
    rng = np.random.default_rng(seed)
    g = (np.zeros(n), np.zeros(n))
    for f in (0, 1):
        g[f][nodes[f]] = rng.uniform(0.5, 1.5, len(nodes[f]))
    return g


def _shifted_context(make, kind, nx, ny, nz, nodes, g, degree=1, options=()):
    ctx = make()
    for name, v in options:
        ctx.set_option(name, v)
    if degree == 1:
        ctx.mesh_build(_dim(kind), kind, nx, ny, nz)
    else:
        ctx.mesh_build_lagrange(_dim(kind), kind, nx, ny, nz, degree)
    for f in (0, 1):
        ctx.set_dirichlet(f, nodes[f], g[f][nodes[f]])
    return ctx


def _compare_assembly(tag, ctx, K, M, masks, g, sigma):
    n = K.shape[0]
    A11, A22, A12, A21, rhs, u0 = T.shifted_blocks(K, M, CF, sigma, masks, g)
    worst = 0.0
    for which, ref in ((_ffi.MAT_A11, A11), (_ffi.MAT_A22, A22), (_ffi.MAT_A12, A12), (_ffi.MAT_A21, A21),
                       (_ffi.MAT_MONO, sp.bmat([[A11, A12], [A21, A22]], format="csr"))):
        got = ctx.csr(which)
        err = abs(got - ref).max() / abs(ref).max()
        worst = max(worst, err)
        assert err <= VAL_TOL, (tag, which, err)
    r, u = ctx.rhs()
    er = abs(r - rhs).max() / max(abs(rhs).max(), 1e-300)
    print(f"{tag}: blocks {worst:.2e}, rhs {er:.2e} (bar {VAL_TOL:g})")
    assert er <= VAL_TOL and np.array_equal(u, u0)


OPTION_SETS = {"default": (), "asm_kernel0": (("asm_kernel", 0),), "asm_kernel1": (("asm_kernel", 1),), "asm_tile2": (("asm_tile", 2),),
               "asm_fused0": (("asm_fused", 0),), "csr": (("op_format", 0),), "store_values": (("asm_store_values", 1),),
               "dicts_split": (("sell_dict_min_rows", 1), ("asm_node_split_min", 16))}


@pytest.mark.parametrize("opts", list(OPTION_SETS))
@pytest.mark.parametrize("sets", ["shared", "mixed"])
@pytest.mark.parametrize("case", SHIFT_CASES, ids=_id)
def test_shifted_assembly_matches_the_restatement(gpu_ctx_factory, case, sets, opts):
    kind, nx, ny, nz = case
    om, K, M = T.scalar_matrices(_dim(kind), kind, nx, ny, nz)
    n = om.num_nodes
    nodes = _dirichlet_sets(kind, nx, ny, nz, sets)
    masks = T.masks_of(n, *nodes)
    g = _dirichlet_data(n, nodes, 3)
    ctx = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, nodes, g, 1, OPTION_SETS[opts])
    ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True, sigma=SIGMA)
    _compare_assembly(f"{_id(case)} {sets} {opts}", ctx, K, M, masks, g, SIGMA)
    # one field shifted, then none: a later assembly is a new system, and sigma = 0 is the plain assembly bit for bit
    ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True, sigma=(0.0, 31.0))
    _compare_assembly(f"{_id(case)} {sets} {opts} (0, 31)", ctx, K, M, masks, g, (0.0, 31.0))
    # (Context.assemble routes sigma = (0, 0) to pph_assemble_dpp: the shifted entry point is called with zeros directly)
    ctx._check(_ffi.lib.pph_assemble_dpp_shifted(ctx._h, CF.k1, CF.k2, CF.beta, CF.mu, 0.0, 0.0, 1))
    a = [ctx.csr(w) for w in (_ffi.MAT_A11, _ffi.MAT_A22, _ffi.MAT_A12, _ffi.MAT_A21, _ffi.MAT_MONO)] + list(ctx.rhs())
    plain = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, nodes, g, 1, OPTION_SETS[opts])
    plain.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True)
    b = [plain.csr(w) for w in (_ffi.MAT_A11, _ffi.MAT_A22, _ffi.MAT_A12, _ffi.MAT_A21, _ffi.MAT_MONO)] + list(plain.rhs())
    # (asm_kernel 0 adds the cells' shares of K and M with floating-point atomics: two assemblies of ONE system already differ
    #  in the last bits there, so that path is compared to 16 eps of the largest entry instead)
    same = np.array_equal if opts != "asm_kernel0" else (lambda u, v: bool(abs(u - v).max() <= 16 * T.EPS * abs(v).max()))
    for x, y in zip(a, b):
        if sp.issparse(x):
            assert np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices) and same(x.data, y.data)
        else:
            assert same(x, y)
    cfg = _cfg(spar.CG_JACOBI_PARAMS)
    if opts != "asm_kernel0":
        assert np.array_equal(ctx.solve(cfg)[0], plain.solve(cfg)[0])


@pytest.mark.parametrize("sets", ["shared", "mixed"])
@pytest.mark.parametrize("case", SHIFT_CASES, ids=_id)
def test_shifted_assembly_at_degree_two(gpu_ctx_factory, case, sets):
    """Degree 2 on the four cell kinds (the two-step path: k_lift_rhs, k_blocks), K and M the context's own exported ones.
    shared: both fields on the whole boundary (A21 aliased to A12, the A21 == nullptr branch of k_blocks); mixed: field 1 on
    the sides x = 0 and y = 0 plus a few interior degree-2 nodes."""
    import p2_restatement as R2

    kind, nx, ny, nz = case
    ctx = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, (np.zeros(0, dtype=np.int64),) * 2, (np.zeros(0), np.zeros(0)), 2)
    n = ctx.n
    K, M = ctx.csr(_ffi.MAT_K), ctx.csr(_ffi.MAT_M)
    bnd = R2.boundary_nodes(kind, nx, ny, nz)
    if sets == "shared":
        nodes = (bnd, bnd)
    else:
        X = R2.coords(kind, nx, ny, nz)
        inner = np.setdiff1d(np.arange(n), bnd)
        nodes = (bnd, np.sort(np.concatenate([bnd[(X[bnd, 0] < 1e-12) | (X[bnd, 1] < 1e-12)], inner[::7]])))
    g = _dirichlet_data(n, nodes, 4)
    for f in (0, 1):
        ctx.set_dirichlet(f, nodes[f], g[f][nodes[f]])
    ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True, sigma=SIGMA)
    _compare_assembly(f"{_id(case)} degree 2 {sets}", ctx, K, M, T.masks_of(n, *nodes), g, SIGMA)


SOLVERS = {"cg_jacobi": (spar.CG_JACOBI_PARAMS, False), "cg_block2": (spar.CG_BLOCK_JACOBI_PARAMS, False),
           "cg_ilu": ({**spar.CG_JACOBI_PARAMS, "pc_type": "ilu", "pc_factor_levels": 0}, False),
           "gmres_ilu": (spar.GMRES_ILU_PARAMS, False), "fieldsplit_mg": (spar.FIELDSPLIT_MG_PARAMS, False),
           "picard_mg": (spar.PICARD_MG_SOLVER_PARAMS, True), "cg_cmg": (spar.CG_CMG_PARAMS, False),
           "fieldsplit_lu": (spar.FIELDSPLIT_LU_PARAMS, False)}


def _direct(K, M, sigma, masks, g):
    import scipy.sparse.linalg as spla

    A11, A22, A12, A21, rhs, u0 = T.shifted_blocks(K, M, CF, sigma, masks, g)
    return spla.spsolve(sp.bmat([[A11, A12], [A21, A22]], format="csc"), rhs) + u0


@pytest.mark.parametrize("name", ["fieldsplit_mg", "picard_mg", "cg_cmg", "cg_ilu", "fieldsplit_lu"])
@pytest.mark.parametrize("case", [(o.CELL_QUAD, 8, 8, 0), (o.CELL_HEX, 4, 4, 4), (o.CELL_TET, 4, 4, 4)], ids=_id)
def test_a_new_sigma_is_a_new_system_for_every_preconditioner(gpu_ctx_factory, case, name):
    """sigma A, solve, sigma B, solve: a hierarchy, dictionary or factorisation that kept the first sigma shows.  The shift
    dominates on the fine level and not on the coarsest (sigma h^2 about 10 k): a level built without it is far off."""
    kind, nx, ny, nz = case
    om, K, M = T.scalar_matrices(_dim(kind), kind, nx, ny, nz)
    n = om.num_nodes
    nodes = _dirichlet_sets(kind, nx, ny, nz, "mixed")
    masks = T.masks_of(n, *nodes)
    g = _dirichlet_data(n, nodes, 5)
    ctx = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, nodes, g, 1, (("sell_dict_min_rows", 1),))
    params, nonlinear = SOLVERS[name]
    cfg = _cfg(params, nonlinear)
    for sigma in ((10.0 * CF.k1 * nx * nx, 10.0 * CF.k2 * nx * nx), (3.0, 0.0), (0.0, 0.0)):
        ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=not cfg.picard, sigma=sigma)
        x, info, _ = ctx.solve(cfg)
        ref = _direct(K, M, sigma, masks, g)
        err = abs(x - ref).max() / abs(ref).max()
        print(f"{_id(case)} {name} sigma {sigma}: {err:.2e}, {info.iterations} iterations")
        assert info.converged and err <= 1e-9


def _initial(om, seed):
    x = om.coords
    rng = np.random.default_rng(seed)
    return np.concatenate([np.cos(2.0 * x[:, 0]) + x[:, 1], 0.3 + 0.5 * np.sin(3.0 * x[:, -1])]) + 0.05 * rng.standard_normal(2 * om.num_nodes)


def _run_steps(ctx, cfg, p0, storage, theta, dt, nsteps, mono=True, **kw):
    ctx.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, storage, theta, dt, monolithic=mono)
    p = p0.copy()
    done, infos, norms = ctx.transient_steps(cfg, p, nsteps, **kw)
    return p, done, infos, norms


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("case", [(o.CELL_QUAD, 4, 4, 0), (o.CELL_HEX, 3, 3, 3)], ids=_id)
def test_stepping_follows_the_closed_form(gpu_ctx_factory, case, theta):
    kind, nx, ny, nz = case
    dim = _dim(kind)
    om = o.build_mesh(dim, kind, nx, ny, nz)
    n = om.num_nodes
    b = o.boundary_nodes(om)
    phi = T.sine_mode(om)
    phi[b] = 0.0
    storage, dt, nsteps = (1.0, 20.0), 0.05, 8
    G = T.amplification(*T.mode_eigenvalues(dim, nx, ny, nz), CF, storage, theta, dt)
    c = T.closed_form_amplitudes(G, (1.0, -0.5), nsteps)[-1]
    ctx = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, (b, b), (np.zeros(n), np.zeros(n)))
    p, done, infos, norms = _run_steps(ctx, _cfg(spar.CG_JACOBI_PARAMS), np.concatenate([phi, -0.5 * phi]), storage, theta, dt, nsteps)
    err = abs(p - np.concatenate([c[0] * phi, c[1] * phi])).max() / abs(phi).max()
    print(f"closed form {_id(case)} theta {theta}: {err:.2e} (bar {STEP_TOL:.1e})")
    assert done == nsteps and all(i.converged for i in infos) and err <= STEP_TOL


STEP_RUNS = [((o.CELL_QUAD, 5, 3, 0), 1, "cg_jacobi"), ((o.CELL_TRI, 4, 3, 0), 1, "cg_block2"), ((o.CELL_HEX, 3, 4, 2), 1, "gmres_ilu"),
             ((o.CELL_TET, 3, 2, 3), 1, "cg_ilu"), ((o.CELL_QUAD, 8, 8, 0), 1, "fieldsplit_mg"), ((o.CELL_HEX, 4, 4, 4), 1, "picard_mg"),
             ((o.CELL_HEX, 4, 4, 4), 1, "cg_cmg"), ((o.CELL_TET, 4, 4, 4), 1, "cg_cmg"), ((o.CELL_QUAD, 8, 8, 0), 1, "fieldsplit_lu"),
             ((o.CELL_QUAD, 4, 4, 0), 2, "pmg")]


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("run", STEP_RUNS, ids=lambda r: f"{_id(r[0])}-deg{r[1]}-{r[2]}")
def test_stepping_matches_the_restatement(gpu_ctx_factory, run, theta):
    """Non-zero Dirichlet data, an initial field that does not match them, every solver family; also: two calls of k steps are
    one call of 2k bit for bit, and the context's right-hand side, lifting and solution come back bit for bit."""
    (kind, nx, ny, nz), degree, name = run
    storage, dt, k = (0.3, 5.0), 0.02, 3
    if degree == 1:
        om, K, M = T.scalar_matrices(_dim(kind), kind, nx, ny, nz)
        n = om.num_nodes
        nodes = _dirichlet_sets(kind, nx, ny, nz, "mixed")
        p0 = _initial(om, 2)
        params, nonlinear = SOLVERS[name]
    else:
        probe = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, (np.zeros(0, dtype=np.int64),) * 2, (np.zeros(0), np.zeros(0)), 2)
        n = probe.n
        K, M = probe.csr(_ffi.MAT_K), probe.csr(_ffi.MAT_M)
        rng = np.random.default_rng(12)
        nodes = (np.sort(rng.choice(n, n // 5, replace=False)), np.sort(rng.choice(n, n // 6, replace=False)))
        p0 = rng.standard_normal(2 * n)
        params, nonlinear = spar.FIELDSPLIT_PMG_PARAMS, False
    masks = T.masks_of(n, *nodes)
    g = _dirichlet_data(n, nodes, 6)
    cfg = _cfg(params, nonlinear)
    mono = not cfg.picard
    ctx = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, nodes, g, degree)
    states, bn, dn = T.theta_steps(K, M, CF, storage, theta, dt, masks, g, p0, 2 * k)
    p, done, infos, norms = _run_steps(ctx, cfg, p0, storage, theta, dt, 2 * k, mono)
    scale = abs(states[-1]).max()
    err = abs(p - states[-1]).max() / scale
    print(f"steps {_id(run[0])} degree {degree} {name} theta {theta}: {err:.2e} (bar {STEP_TOL:.1e}), iterations {[i.iterations for i in infos]}")
    assert done == 2 * k and all(i.converged for i in infos)
    assert err <= STEP_TOL
    assert np.allclose(norms[:, 0], bn, rtol=1e-8, atol=0) and np.allclose(norms[:, 1], dn, rtol=1e-8, atol=0)
    assert np.array_equal(p[np.concatenate(masks)], np.concatenate(g)[np.concatenate(masks)])
    # k + k = 2k, bit for bit; the context's vectors restored
    before = ctx.rhs() + (ctx.solution().copy(),)
    q = p0.copy()
    d1, _, n1 = ctx.transient_steps(cfg, q, k)
    d2, _, n2 = ctx.transient_steps(cfg, q, k)
    assert d1 == d2 == k and np.array_equal(q, p) and np.array_equal(np.vstack([n1, n2]), norms)
    after = ctx.rhs() + (ctx.solution().copy(),)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    qd = torch.from_numpy(p0.copy()).cuda()   # the device variant: the same bits
    d3, _, n3 = ctx.transient_steps(cfg, qd, 2 * k)
    assert d3 == 2 * k and np.array_equal(qd.cpu().numpy(), p) and np.array_equal(n3, norms)


def test_steady_tol_zero_rhs_and_balance(gpu_ctx_factory):
    kind, nx, ny, nz = o.CELL_QUAD, 5, 3, 0
    om, K, M = T.scalar_matrices(2, kind, nx, ny, nz)
    n = om.num_nodes
    nodes = _dirichlet_sets(kind, nx, ny, nz, "mixed")
    masks = T.masks_of(n, *nodes)
    con = np.concatenate(masks)
    g = _dirichlet_data(n, nodes, 6)
    storage, dt = (0.3, 5.0), 0.5
    cfg = _cfg(spar.CG_JACOBI_PARAMS)
    ctx = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, nodes, g)
    p0 = _initial(om, 2)
    # steady_tol stops where the restatement's norms say
    states, bn, dn = T.theta_steps(K, M, CF, storage, 1.0, dt, masks, g, p0, 40, steady_tol=1e-3)
    assert 2 < len(bn) < 40
    p, done, infos, norms = _run_steps(ctx, cfg, p0, storage, 1.0, dt, 40, steady_tol=1e-3)
    print(f"steady_tol: stopped after {done} steps (restatement {len(bn)})")
    assert done == len(bn) and abs(p - states[-1]).max() <= STEP_TOL * abs(states[-1]).max()
    # balance identity after ONE backward-Euler step: Sigma M (p1 - p0) / dt + A_unel p1 is, on the free dofs, minus the residual
    # of the step's solve.  CG + Jacobi reports the PRECONDITIONED norm ||D^-1 r||_2 of its recurrence residual (D the diagonal
    # of the step operator), so that is the norm recomputed here.  The solve stops at rtol 1e-6: its residual is then nine
    # decades above the rounding of either side (eps ||D^-1 b||, times the condition number for the drift of CG's recurrence: at
    # most 1e-14 ||D^-1 b|| here against a resnorm above 1e-9 ||D^-1 b||), and the recomputed norm must equal the reported one to 1e-4
    # relative - a stale, zero or otherwise foreign resnorm cannot.
    loose = _cfg(spar.CG_JACOBI_PARAMS)
    loose.rtol = 1e-6
    q = p0.copy()
    d, infos, norms = ctx.transient_steps(loose, q, 1)
    dinv = 1.0 / np.concatenate([ctx.csr(_ffi.MAT_A11).diagonal(), ctx.csr(_ffi.MAT_A22).diagonal()])
    start = np.where(con, np.concatenate(g), p0)
    inc = (q - start) / dt
    bal = np.concatenate([storage[0] * ctx.spmv(_ffi.MAT_M, inc[:n]), storage[1] * ctx.spmv(_ffi.MAT_M, inc[n:])]) \
        + ctx.dpp_nodal_flux(q, CF.k1, CF.k2, CF.beta, CF.mu)
    res = float(np.linalg.norm((dinv * bal)[~con]))
    bpre = float(np.linalg.norm((dinv * ctx.step_rhs(start, CF.k1, CF.k2, CF.beta, CF.mu))[~con]))
    print(f"balance: ||D^-1 (balance on free dofs)|| {res:.6e}, solver's resnorm {infos[0].resnorm:.6e}, ||D^-1 b|| {bpre:.3e}, "
          f"{infos[0].iterations} iterations")
    assert d == 1 and infos[0].converged and infos[0].iterations > 0
    assert 1e-9 * bpre < infos[0].resnorm <= 1e-6 * bpre
    assert abs(res - infos[0].resnorm) <= 1e-4 * infos[0].resnorm
    assert abs(norms[0, 0] - np.linalg.norm(ctx.step_rhs(start, CF.k1, CF.k2, CF.beta, CF.mu))) <= 1e-13 * norms[0, 0]
    # a right-hand side that is zero on every free dof takes no solve: homogeneous data, and an initial field that is non-zero
    # on constrained dofs only (they are overwritten first)
    flat = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, nodes, (np.zeros(n), np.zeros(n)))
    z = np.where(con, 3.0, 0.0)
    flat.transient_begin(CF.k1, CF.k2, CF.beta, CF.mu, storage, 1.0, dt)
    d, infos, norms = flat.transient_steps(cfg, z, 3)
    assert d == 3 and all(i.iterations == 0 and i.converged for i in infos) and np.all(norms == 0.0)
    assert np.all(z == 0.0)


def test_transient_refusals_leave_the_context_usable(gpu_ctx_factory):
    kind, nx, ny = o.CELL_QUAD, 4, 4
    om = o.build_mesh(2, kind, nx, ny)
    n = om.num_nodes
    b = o.boundary_nodes(om)
    ctx = _shifted_context(gpu_ctx_factory, kind, nx, ny, 0, (b, b), (np.zeros(n), np.zeros(n)))
    cfg = _cfg(spar.CG_JACOBI_PARAMS)
    p = np.ones(2 * n)
    with pytest.raises(ValueError, match="before pph_transient_begin"):
        ctx.transient_steps(cfg, p, 1)
    for bad in ((-1.0, 0.0), (0.0, float("nan")), (float("inf"), 1.0)):
        with pytest.raises(ValueError, match="sigma"):
            ctx.assemble(1.0, 1.0, 1.0, 1.0, sigma=bad)
    for storage, theta, dt, msg in (((0.0, 1.0), 1.0, 0.1, "storage"), ((1.0, -1.0), 1.0, 0.1, "storage"), ((1.0, 1.0), 0.4, 0.1, "theta"),
                                    ((1.0, 1.0), 1.1, 0.1, "theta"), ((1.0, 1.0), 1.0, 0.0, "dt"), ((1.0, 1.0), 1.0, float("nan"), "dt")):
        with pytest.raises(ValueError, match=msg):
            ctx.transient_begin(1.0, 1.0, 1.0, 1.0, storage, theta, dt)
    ctx.transient_begin(1.0, 0.5, 2.0, 1.0, (1.0, 2.0), 1.0, 0.1)
    with pytest.raises(ValueError, match="nsteps"):
        ctx.transient_steps(cfg, p, 0)
    done = C.c_int(0)
    assert _ffi.lib.pph_transient_steps(ctx._h, C.byref(cfg), None, 1, 0.0, None, None, C.byref(done)) == _ffi.PPH_ERR_INVALID
    assert b"NULL buffer" in _ffi.lib.pph_last_error(ctx._h)
    assert _ffi.lib.pph_transient_steps_device(ctx._h, C.byref(cfg), None, 1, 0.0, None, None, C.byref(done)) == _ffi.PPH_ERR_INVALID
    ctx.assemble(1.0, 0.5, 2.0, 1.0)
    with pytest.raises(ValueError, match="assembled again"):
        ctx.transient_steps(cfg, p, 1)
    ctx.transient_begin(1.0, 0.5, 2.0, 1.0, (1.0, 2.0), 1.0, 0.1)
    ctx.set_dirichlet(1, b[:-1], np.zeros(len(b) - 1))
    with pytest.raises(ValueError, match="assembled again|Dirichlet sets changed"):
        ctx.transient_steps(cfg, p, 1)
    # ... and still works
    ctx.transient_begin(1.0, 0.5, 2.0, 1.0, (1.0, 2.0), 1.0, 0.1)
    d, infos, norms = ctx.transient_steps(cfg, p, 2)
    assert d == 2 and all(i.converged for i in infos) and np.all(np.isfinite(p))


# -- preconditioners see the shift: one application each against restated cycles -----------------------------------------
import mg_cycle_reference as MC  # noqa: E402
import pmg_restatement as PM  # noqa: E402
from oracle import dpp_mg_oracle as GO  # noqa: E402

PC_CASES = [(o.CELL_QUAD, 8, 8, 0), (o.CELL_HEX, 4, 4, 4), (o.CELL_TET, 4, 4, 4)]


def _dominant_sigma(nx):
    """sigma h_fine^2 about 10 k: the shift dominates on the fine level and not on the coarsest - a level built without it is
    far outside the per-application bounds."""
    return (10.0 * CF.k1 / CF.mu * nx * nx, 10.0 * CF.k2 / CF.mu * nx * nx)


@pytest.mark.parametrize("sets", ["shared", "mixed"])
@pytest.mark.parametrize("case", PC_CASES, ids=_id)
def test_block_preconditioners_see_the_shift(gpu_ctx_factory, case, sets):
    """pph_pc_apply (Jacobi, multigrid, ILU) on a shifted system against restated applications, to the per-application bound
    of tests/test_mg_cycle_gpu.py (mg_cycle_reference.CYCLE_BOUND); a cycle restated WITHOUT the shift is far outside it."""
    kind, nx, ny, nz = case
    om, K, M = T.scalar_matrices(_dim(kind), kind, nx, ny, nz)
    n = om.num_nodes
    nodes = _dirichlet_sets(kind, nx, ny, nz, sets)
    masks = T.masks_of(n, *nodes)
    g = _dirichlet_data(n, nodes, 9)
    sigma = _dominant_sigma(nx)
    ctx = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, nodes, g)
    ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=False, sigma=sigma)
    A11, A22, _, _, _, _ = T.shifted_blocks(K, M, CF, sigma, masks, g)
    a, b, c = CF.abc
    rng = np.random.default_rng(17)
    for which, (A, cK) in enumerate(((A11, a), (A22, c))):
        mask = masks[which]
        lv = GO.build_hierarchy(_dim(kind), kind, nx, ny, nz, cK, b + sigma[which], mask)
        plain = GO.build_hierarchy(_dim(kind), kind, nx, ny, nz, cK, b, mask)
        r = rng.standard_normal(n)
        rm = np.where(mask, 0.0, r)
        for ns in (1, 2):
            ref = MC.apply_reference(lv, rm, ns)
            z = ctx.pc_apply(which, _ffi.PC_MG, r, mg_smooth=ns)
            err, off = MC.rel_err(z, ref), MC.rel_err(MC.apply_reference(plain, rm, ns), ref)
            print(f"{_id(case)} {sets} block {which} mg_smooth {ns}: |z - ref| / |ref| = {err:.2e} (bound {MC.CYCLE_BOUND:.0e}); unshifted cycle {off:.2e}")
            assert err <= MC.CYCLE_BOUND and off > 1e3 * MC.CYCLE_BOUND and not z[mask].any()
        zj = ctx.pc_apply(which, _ffi.PC_JACOBI, r)
        assert MC.rel_err(zj, rm / A.diagonal()) <= 1e-14
        zi = ctx.pc_apply(which, _ffi.PC_ILU, r)
        assert MC.rel_err(zi, o.ilu0_apply(A.tocsr())(rm)) <= 1e-12


@pytest.mark.parametrize("sets", ["shared", "mixed"])
@pytest.mark.parametrize("case", PC_CASES, ids=_id)
def test_coupled_preconditioners_see_the_shift(gpu_ctx_factory, case, sets):
    """pph_pc_apply_coupled (coupled multigrid, block-2 Jacobi, Jacobi) against tests/cmg_reference.py's cycle on the
    hierarchy with per-field mass coefficients (transient_reference.coupled_hierarchy_shifted), to its bound."""
    kind, nx, ny, nz = case
    om, K, M = T.scalar_matrices(_dim(kind), kind, nx, ny, nz)
    n = om.num_nodes
    nodes = _dirichlet_sets(kind, nx, ny, nz, sets)
    masks = T.masks_of(n, *nodes)
    con = np.concatenate(masks)
    g = _dirichlet_data(n, nodes, 9)
    sigma = _dominant_sigma(nx)
    ctx = _shifted_context(gpu_ctx_factory, kind, nx, ny, nz, nodes, g)
    ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=True, sigma=sigma)
    lv = T.coupled_hierarchy_shifted(kind, nx, ny, nz, masks, CF, sigma)
    plain = T.coupled_hierarchy_shifted(kind, nx, ny, nz, masks, CF, (0.0, 0.0))
    r = np.random.default_rng(19).standard_normal(2 * n)
    rm = np.where(con, 0.0, r)
    for ns in (1, 2):
        ref = CR.apply_reference(lv, rm, ns)
        z = ctx.pc_apply_coupled(_ffi.PC_CMG, r, mg_smooth=ns)
        err, off = CR.rel_err(z, ref), CR.rel_err(CR.apply_reference(plain, rm, ns), ref)
        print(f"{_id(case)} {sets} coupled mg_smooth {ns}: |z - ref| / |ref| = {err:.2e} (bound {CR.CYCLE_BOUND:.0e}); unshifted cycle {off:.2e}")
        assert err <= CR.CYCLE_BOUND and off > 1e3 * CR.CYCLE_BOUND and not z[con].any()
    A = lv[0].A
    assert CR.rel_err(ctx.pc_apply_coupled(_ffi.PC_BLOCK2, r), CR.dinv_apply(lv[0], rm)) <= 1e-13
    assert CR.rel_err(ctx.pc_apply_coupled(_ffi.PC_JACOBI, r), rm / A.diagonal()) <= 1e-14


@pytest.mark.parametrize("case", [(o.CELL_QUAD, 8, 8, 0), (o.CELL_HEX, 4, 4, 4)], ids=_id)
def test_p_multigrid_sees_the_shift_at_degree_two(gpu_ctx_factory, case):
    """pph_pc_apply (pph_pmg) on a degree-2 shifted system against tests/pmg_restatement.py, bound of tests/test_pmg_gpu.py."""
    import p2_restatement as R2

    kind, nx, ny, nz = case
    ctx = gpu_ctx_factory()
    ctx.mesh_build_lagrange(_dim(kind), kind, nx, ny, nz, 2)
    bnd = R2.boundary_nodes(kind, nx, ny, nz)
    mask = np.zeros(ctx.n, bool)
    mask[bnd] = True
    for f in (0, 1):
        ctx.set_dirichlet(f, bnd, np.full(len(bnd), 1.0 + f))
    sigma = _dominant_sigma(2 * nx)
    ctx.assemble(CF.k1, CF.k2, CF.beta, CF.mu, monolithic=False, sigma=sigma)
    a, b, c = CF.abc
    rng = np.random.default_rng(23)
    for which, cK in ((0, a), (1, c)):
        lv = PM.build_levels(kind, nx, ny, nz, cK, b + sigma[which], mask)
        plain = PM.build_levels(kind, nx, ny, nz, cK, b, mask)
        for ns in (1, 2):
            r = rng.standard_normal(ctx.n)
            rm = np.where(mask, 0.0, r)
            ref = PM.cycle(lv, rm, ns)
            z = ctx.pc_apply(which, _ffi.PC_PMG, r, mg_smooth=ns)
            err, off = abs(z - ref).max() / abs(ref).max(), abs(PM.cycle(plain, rm, ns) - ref).max() / abs(ref).max()
            print(f"{_id(case)} degree 2 block {which} mg_smooth {ns}: {err:.2e} (bound 1e-10); unshifted cycle {off:.2e}")
            assert err <= 1e-10 and off > 1e-7 and not z[mask].any()


def test_c_abi_refuses_slab_contexts():
    """Two ranks over gloo, each with its slab of a distributed mesh (world = 2): pph_dpp_step_rhs*, pph_assemble_dpp_shifted
    with a sigma != 0, pph_transient_begin and pph_transient_steps* return PPH_ERR_INVALID with their message, and
    solve_dpp_transient raises NotImplementedError before any of them (tools/transient_slab_check.py)."""
    import socket
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tools", "transient_slab_check.py")]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0 and "world=2 transient refusals: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# -- the public function ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_solve_dpp_transient_observes_and_records(on_device):
    import perphil_amd as pa
    from perphil_amd import fd

    kind, nx, ny = o.CELL_QUAD, 6, 5
    om, K, M = T.scalar_matrices(2, kind, nx, ny)
    n = om.num_nodes
    b = o.boundary_nodes(om)
    masks = T.masks_of(n, b, b)
    g = (np.where(masks[0], 1.0 + om.coords[:, 0], 0.0), np.where(masks[1], 0.5 - om.coords[:, 1], 0.0))
    mesh = fd.Mesh(2, kind, nx, ny, 0, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    bcs = [fd.DirichletBC(W.sub(0), g[0].copy()), fd.DirichletBC(W.sub(1), g[1].copy())]
    params = pa.DPPParameters(k1=CF.k1, k2=CF.k2, beta=CF.beta, mu=CF.mu)
    init = (lambda X: np.cos(2.0 * X[:, 0]) + X[:, 1], lambda X: 0.3 + 0.5 * np.sin(3.0 * X[:, 1]))
    p0 = np.concatenate([init[0](om.coords), init[1](om.coords)])
    pts = np.array([[0.5, 0.5], [0.21, 0.77], [0.9, 0.05], [0.0, 1.0]])
    storage, theta, dt, nsteps = (0.3, 5.0), 0.5, 0.02, 5
    sp_ = {**spar.CG_JACOBI_PARAMS, "ksp_rtol": 1e-12, "ksp_atol": 1e-300}
    ts = pa.solve_dpp_transient(W, params, bcs, init, dt, nsteps, storage=storage, theta=theta, solver_parameters=sp_,
                                observe_at=pts, record_every=2, on_device=on_device)
    states, bn, dn = T.theta_steps(K, M, CF, storage, theta, dt, masks, g, p0, nsteps)
    assert ts.steps_done == nsteps and np.allclose(ts.times, dt * np.arange(nsteps + 1))
    assert ts.iterations.shape == ts.rhs_norms.shape == ts.increment_norms.shape == (nsteps,) and ts.observations.shape == (nsteps + 1, 4, 2)
    assert sorted(ts.snapshots) == [0, 2, 4, 5] and ts.solution.on_device == on_device
    assert abs(ts.solution.vector() - states[-1]).max() <= STEP_TOL * abs(states[-1]).max()
    assert np.allclose(ts.rhs_norms, bn, rtol=1e-8, atol=0) and np.allclose(ts.increment_norms, dn, rtol=1e-8, atol=0)
    for step, f in ts.snapshots.items():
        assert abs(f.vector() - states[step]).max() <= STEP_TOL * abs(states[step]).max()
        for fld in (0, 1):
            at = np.asarray(f.sub(fld).at(pts)).reshape(-1)
            assert np.array_equal(at, ts.observations[step, :, fld]), (step, fld)
    # the steady-state stop, through the chunks of one step each that observing takes
    stop = pa.solve_dpp_transient(W, params, bcs, init, 0.5, 60, storage=storage, theta=1.0, solver_parameters=sp_, observe_at=pts,
                                  steady_tol=1e-3)
    ref = T.theta_steps(K, M, CF, storage, 1.0, 0.5, masks, g, p0, 60, steady_tol=1e-3)
    assert stop.steps_done == len(ref[1]) < 60 and stop.observations.shape[0] == stop.steps_done + 1
