"""Adjoint solves and sensitivities on the device (pph_adjoint.hip through perphil_amd.adjoint and the context methods)
against the NumPy restatement of tests/adjoint_reference.py, which tests/test_adjoint_host.py pins against difference
quotients.

Bars.  Bilinear forms on given fields: 1e-12 of each term's sum of the absolute values of the products added, the project's
bar wherever only the order of summation differs.  Closed forms: 1e-13 of the scale stated with them.  pph_solve_rhs behind a
direct-equivalent solve: 1e-10 of max |x|, the project's bar there (test_mass_balance_gpu.py).  Sensitivities end to end:
the test's docstring.  Every test prints its worst figure before it asserts."""
import ctypes as C
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import perphil_amd as pa  # noqa: E402
from perphil_amd import _ffi, adjoint, fd, solver, solver_parameters as spar  # noqa: E402
import adjoint_reference as AR  # noqa: E402
import flux_reference as FR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES2, SHAPES3 = [(5, 3, 0), (2, 2, 0), (1, 3, 0), (300, 4, 0)], [(3, 4, 2), (2, 2, 2), (20, 17, 2)]
CASES = [(k, deg) + s for k in (FR.QUAD, FR.TRI, FR.HEX, FR.TET) for deg in (1, 2)
         for s in (SHAPES2 if k in (FR.QUAD, FR.TRI) else SHAPES3)]
IDS = [f"{AR.NAMES[c[0]]}{c[2]}x{c[3]}x{c[4]}-deg{c[1]}" for c in CASES]
GMRES_ILU_TIGHT = dict(spar.GMRES_ILU_PARAMS, ksp_rtol=1e-12)
GMRES_FIELDSPLIT_LU = {**spar.GMRES_PARAMS, **spar.FIELDSPLIT_LU_PARAMS}


def _spaces(kind, deg, nx, ny, nz):
    mesh = fd.Mesh(FR.dim_of(kind), kind, nx, ny, nz, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(mesh, "CG", deg)
    return mesh, V, V * V


def _context(mesh, deg):
    return mesh.context(degree=deg) if deg != 1 else mesh.context()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).copy()).cuda()


# ---- the bilinear forms ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random(case):
    """Two random mixed fields of a case, the restatement's terms and the device's (two calls), computed once."""
    kind, deg, nx, ny, nz = case
    s = FR.space(kind, deg, nx, ny, nz)
    rng = np.random.default_rng(2000 + CASES.index(case))
    lam, p = rng.standard_normal(2 * s.n), rng.standard_normal(2 * s.n)
    ref = AR.bilinear(s, lam, p)
    mesh, _, _ = _spaces(kind, deg, nx, ny, nz)
    ctx = _context(mesh, deg)
    dl, dp = _cuda(lam), _cuda(p)
    before = dict(_ffi.fetch_stats)
    gpu = [ctx.dpp_bilinear(dl, dp) for _ in range(2)]
    assert _ffi.fetch_stats == before
    return s, lam, p, ref, gpu, ctx


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bilinear_forms_of_random_fields(case):
    s, lam, p, (terms, absn), gpu, ctx = _random(case)
    err = [abs(g - t) / a for g, t, a in zip(gpu[0], terms, absn)]
    print(f"bilinear {IDS[CASES.index(case)]}: {err[0]:.2e}, {err[1]:.2e}, {err[2]:.2e} of the absolute sums (bar 1e-12)")
    assert max(err) <= 1e-12
    assert gpu[0] == gpu[1]                               # the second call: the same bits
    assert ctx.dpp_bilinear(lam, p) == gpu[0]             # host fields, uploaded for the call: the same bits


CLOSED = [c for c in CASES if c[2:] in ((5, 3, 0), (3, 4, 2), (20, 17, 2))]


@pytest.mark.parametrize("case", CLOSED, ids=[IDS[CASES.index(c)] for c in CLOSED])
def test_bilinear_closed_forms(case):
    """lam1 = a.x + c, p1 = b.x + c': o0 = a.b (bar 1e-13 |a| |b|); lam1 - lam2 = 1, p1 - p2 = a.x + c: o2 = sum(a) / 2 + c
    (bar 1e-13 (sum |a| + |c|)).  nx != ny != nz: an axis mix-up shows.  The shapes stop at 20 x 17 x 2: the nodal values
    fl(a.x + c) carry a rounding of eps |u| each, a stiffness form differentiates them twice over - its products are
    (deg n)^2 times the result - and so the closed form of o0 holds to about eps (deg n)^2 only, whatever the order of the
    sums: 1.2e-15 measured at 5 x 3, degree 2, 4.4e-12 at 300 x 4 ((600 / 10)^2 times that), 2e-14 expected at 20 x 17 x 2.
    The 300 x 4 shapes are held to the restatement, relative to their products, in test_bilinear_forms_of_random_fields."""
    kind, deg, nx, ny, nz = case
    mesh, _, _ = _spaces(kind, deg, nx, ny, nz)
    d = mesh.dim
    ctx = _context(mesh, deg)
    X = mesh.node_coordinates(degree=deg)
    a, b, c, c2 = np.array([1.5, -2.0, 0.75])[:d], np.array([0.4, 1.25, -3.0])[:d], 0.3, -1.1
    n = X.shape[0]
    lam = np.concatenate([X @ a + c, 2.0 * (X @ b) - c2])
    p = np.concatenate([X @ b + c2, 0.5 * (X @ a) + c])
    o0, o1, _ = ctx.dpp_bilinear(_cuda(lam), _cuda(p))
    e0 = abs(o0 - a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
    e1 = abs(o1 - a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))      # (2 b) . (a / 2)
    # lam2 random on the grid 2^-20 (lam2 + 1 is then exact), p2 random: forming p2 + (a.x + c) rounds by at most
    # eps max |p1| = 1e-15, two orders below the bar
    rng = np.random.default_rng(7)
    l2, p2 = np.round(rng.uniform(-1.0, 1.0, n) * 2.0 ** 20) / 2.0 ** 20, rng.standard_normal(n)
    lam = np.concatenate([l2 + 1.0, l2])
    p = np.concatenate([p2 + (X @ a + c), p2])
    _, _, o2 = ctx.dpp_bilinear(_cuda(lam), _cuda(p))
    e2 = abs(o2 - (a.sum() / 2 + c)) / (np.abs(a).sum() + abs(c))
    print(f"closed forms {IDS[CASES.index(case)]}: o0 {e0:.2e}, o1 {e1:.2e}, o2 {e2:.2e} (bar 1e-13)")
    assert e0 <= 1e-13 and e1 <= 1e-13 and e2 <= 1e-13


# ---- pph_solve_rhs -----------------------------------------------------------------------------------------------------
def _assembled(kind, deg, n, opts, params=(1.0, 0.01, 1.0, 1.0), nonlinear=False):
    d = FR.dim_of(kind)
    mesh, V, W = _spaces(kind, deg, n, n, n if d == 3 else 0)
    s = FR.space(kind, deg, n, n, n if d == 3 else 0)
    g = AR.smooth_boundary_data(s)
    bcs = [fd.DirichletBC(W.sub(0), g[:s.n].copy()), fd.DirichletBC(W.sub(1), g[s.n:].copy())]
    P = pa.DPPParameters(k1=params[0], k2=params[1], beta=params[2], mu=params[3])
    cfg, info = solver.translate_options(opts, nonlinear=nonlinear)
    ctx = _context(mesh, deg)
    solver._apply_bcs(ctx, W, bcs)
    ctx.assemble(*params, monolithic=not cfg.picard)
    return s, W, bcs, P, cfg, ctx, g


@pytest.mark.parametrize("kind,deg,n,opts", [(FR.QUAD, 1, 8, spar.LINEAR_SOLVER_PARAMS), (FR.HEX, 1, 4, spar.LINEAR_SOLVER_PARAMS),
                                             (FR.QUAD, 2, 8, GMRES_ILU_TIGHT)], ids=["quad8-deg1-lu", "hex4-deg1-lu", "quad8-deg2-ilu"])
def test_solve_rhs_against_the_direct_solve(kind, deg, n, opts):
    params = (1.0, 0.01, 1.0, 1.0)
    s, W, bcs, P, cfg, ctx, g = _assembled(kind, deg, n, opts, params)
    rng = np.random.default_rng(31)
    b = rng.standard_normal(2 * s.n)
    want = AR.solve_free(s, *params, b)
    x, info, _ = ctx.solve_rhs(cfg, _cuda(b))
    xh = x.cpu().numpy()
    err = np.abs(xh - want).max() / np.abs(want).max()
    print(f"solve_rhs: {err:.2e} of max |x| (bar 1e-10), {info.iterations} iterations, converged {info.converged}")
    assert info.converged == 1 and err <= 1e-10
    cd = AR.constrained_dofs(s)
    assert np.all(xh[cd] == 0.0)
    # entries of b on constrained dofs change no bit
    b2 = b.copy()
    b2[cd] = rng.standard_normal(cd.size) * 1e3
    x2, _, _ = ctx.solve_rhs(cfg, _cuda(b2))
    assert torch.equal(x, x2)
    # the host variant: the same bits
    x3, _, _ = ctx.solve_rhs(cfg, b)
    assert np.array_equal(x3, xh)
    # a right-hand side that is zero on every free dof
    z = np.zeros(2 * s.n)
    z[cd] = 1.0
    x0, i0, _ = ctx.solve_rhs(cfg, _cuda(z))
    assert float(x0.abs().max()) == 0.0 and i0.iterations == 0 and i0.converged == 1
    # b and x must differ
    t = _cuda(b)
    st = _ffi.lib.pph_solve_rhs_device(ctx._h, C.byref(cfg), C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr()), None, None, 0)
    assert st == _ffi.PPH_ERR_INVALID and "different buffers" in (_ffi.lib.pph_last_error(ctx._h) or b"").decode()


STATE_OPTS = [("cg-cmg", spar.CG_CMG_PARAMS, False, 0), ("gmres-fieldsplit-lu", GMRES_FIELDSPLIT_LU, False, 0),
              ("picard-mg", spar.PICARD_MG_SOLVER_PARAMS, True, 0), ("picard-mg-fixed-graphs", spar.PICARD_MG_FIXED_SOLVER_PARAMS, True, 2)]


@pytest.mark.parametrize("name,opts,nonlinear,graphs", STATE_OPTS, ids=[o[0] for o in STATE_OPTS])
def test_solve_rhs_preserves_the_context(name, opts, nonlinear, graphs):
    """Forward solve, rhs solve, forward solve on hexahedra 16^3: the context's right-hand side, lifting and solution hold
    the same bits after the rhs solve, and the second forward solve returns the bits of the first (the last preset replays
    its sweeps from captured graphs, which hold the buffers' addresses)."""
    s, W, bcs, P, cfg, ctx, g = _assembled(FR.HEX, 1, 16, opts, nonlinear=nonlinear)
    if graphs:
        ctx.set_option("use_graphs", graphs)
    try:
        _, i1, _ = ctx.solve(cfg, fetch=False)
        first = ctx.solution_tensor()
        rhs0, u00 = ctx.rhs()
        b = _cuda(np.random.default_rng(3).standard_normal(2 * s.n))
        x, ia, _ = ctx.solve_rhs(cfg, b)
        assert ia.converged == 1 and float(x.abs().max()) > 0.0
        rhs1, u01 = ctx.rhs()
        assert np.array_equal(rhs0, rhs1) and np.array_equal(u00, u01)
        assert torch.equal(ctx.solution_tensor(), first)
        _, i2, _ = ctx.solve(cfg, fetch=False)
        again = ctx.solution_tensor()
        print(f"{name}: forward {i1.iterations} its, rhs solve {ia.iterations} its, forward again {i2.iterations} its, "
              f"max |difference| {float((again - first).abs().max()):.1e}")
        assert torch.equal(again, first) and i1.iterations == i2.iterations
        # and the rhs solve does what it says
        want = AR.solve_free(s, 1.0, 0.01, 1.0, 1.0, b.cpu().numpy())
        err = float(np.abs(x.cpu().numpy() - want).max() / np.abs(want).max())
        print(f"   rhs solve against the direct solve: {err:.2e} of max |x|")
        assert err <= 1e-5       # (the presets' own tolerances, 1e-8 on the residual: not the test's subject)
    finally:
        if graphs:
            ctx.set_option("use_graphs", 1)


# ---- sensitivities end to end ------------------------------------------------------------------------------------------------
SENS_CASES = [(FR.QUAD, 5, 3, 0), (FR.TRI, 4, 3, 0), (FR.HEX, 3, 4, 2), (FR.TET, 2, 3, 2)]


def _problem(case, params):
    kind, nx, ny, nz = case
    mesh, V, W = _spaces(kind, 1, nx, ny, nz)
    s = FR.space(kind, 1, nx, ny, nz)
    g = AR.smooth_boundary_data(s)
    w, d = AR.functional_data(s, 11)
    P = pa.DPPParameters(k1=params[0], k2=params[1], beta=params[2], mu=params[3])
    return s, W, g, w, d, P


@pytest.mark.parametrize("params", AR.PARAM_SETS, ids=["k2=1e-2,beta=1,mu=1", "k2=1e-2,beta=3,mu=2", "k2=1e-4,beta=100,mu=1"])
@pytest.mark.parametrize("case", SENS_CASES, ids=["quad5x3", "tri4x3", "hex3x4x2", "tet2x3x2"])
def test_sensitivities_against_the_restatement(case, params):
    """solve_dpp, then sensitivities(wrt_bcs=True), with the direct-equivalent options at degree 1, against the restatement's
    own direct solves: the three terms relative to their absolute sums, the adjoint and the boundary gradient relative to
    their largest entry, and the mu identity |dJ/dmu| <= 1e-10 (|k1 o0| + |k2 o1| + |beta o2|) / mu^2 on the device's own
    terms.  Bar: the larger of 1e-10 and 10 x what the restatement itself loses when both of its solves run by the oracle's
    pcg at rtol 1e-13 instead of spsolve.  Measured on the CPU for these meshes and parameter sets: at most 1.3e-14 (terms),
    1.2e-14 (boundary gradient), 2.7e-14 (adjoint); 10 x that is below 1e-10, so the bar is 1e-10."""
    s, W, g, w, d, P = _problem(case, params)
    bcs = [fd.DirichletBC(W.sub(0), g[:s.n].copy()), fd.DirichletBC(W.sub(1), g[s.n:].copy())]
    sol = pa.solve_dpp(W, P, bcs, solver_parameters=spar.LINEAR_SOLVER_PARAMS)
    p = sol.solution.torch()
    assert p.is_cuda
    gJ = _cuda(w) * (p - _cuda(d))
    before = dict(_ffi.fetch_stats)
    sens = adjoint.sensitivities(W, P, bcs, sol.solution, gJ, spar.LINEAR_SOLVER_PARAMS, wrt_bcs=True)
    assert _ffi.fetch_stats == before and sens.adjoint.on_device and all(f.on_device for f in sens.bcs)
    assert sens.info["converged"] and isinstance(sens, adjoint.Sensitivities)
    p0 = AR.forward(s, *params, g)
    ref = AR.sensitivities(s, *params, p0, AR.dJ_of(p0, w, d))
    et = max(abs(a - b) / sc for a, b, sc in zip(sens.terms, ref.terms, ref.abs_terms))
    lam = sens.adjoint.torch().cpu().numpy()
    el = np.abs(lam - ref.lam).max() / np.abs(ref.lam).max()
    bc = np.concatenate([f.torch().cpu().numpy() for f in sens.bcs])
    eb = np.abs(bc - ref.bcs).max() / np.abs(ref.bcs).max()
    k1, k2, beta, mu = params
    o0, o1, o2 = sens.terms
    scale = (abs(k1 * o0) + abs(k2 * o1) + abs(beta * o2)) / mu ** 2
    print(f"sensitivities: terms {et:.2e}, adjoint {el:.2e}, boundary gradient {eb:.2e} (bar 1e-10); dJ/dmu {sens.mu:.2e} of "
          f"scale {scale:.2e}; solution {float(np.abs(p.cpu().numpy() - p0).max() / np.abs(p0).max()):.2e}")
    assert et <= 1e-10 and el <= 1e-10 and eb <= 1e-10
    assert abs(sens.mu) <= 1e-10 * scale
    assert sens.k1 == -o0 / mu and sens.k2 == -o1 / mu and sens.beta == -o2 / mu
    cd = AR.constrained_dofs(s)
    assert np.all(lam[cd] == 0.0) and np.all(bc[AR.free_dofs(s)] == 0.0)


# ---- autograd --------------------------------------------------------------------------------------------------------------
def test_autograd_equals_the_explicit_sensitivities():
    case, params = (FR.HEX, 3, 4, 2), (1.0, 0.01, 3.0, 2.0)
    s, W, g, w, d, P = _problem(case, params)
    wt, dt = _cuda(w), _cuda(d)
    k1, k2, beta, mu = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in params)
    g0 = _cuda(g[:s.n]).requires_grad_()
    bcs = [fd.DirichletBC(W.sub(0), g0), fd.DirichletBC(W.sub(1), g[s.n:].copy())]
    p = adjoint.solve_dpp_torch(W, k1, k2, beta, mu, bcs, spar.LINEAR_SOLVER_PARAMS)
    assert p.is_cuda and p.shape == (2 * s.n,) and p.requires_grad
    J = 0.5 * torch.sum(wt * (p - dt) ** 2)
    # a forward solve with other parameters and other boundary data in between
    other = [fd.DirichletBC(W.sub(0), 2.0), fd.DirichletBC(W.sub(1), -1.0)]
    pa.solve_dpp(W, pa.DPPParameters(k1=2.0, k2=0.5, beta=0.1, mu=1.0), other, solver_parameters=spar.LINEAR_SOLVER_PARAMS)
    before = dict(_ffi.fetch_stats)
    J.backward()
    assert _ffi.fetch_stats == before
    # the explicit call on the same numbers
    q = p.detach().clone().requires_grad_()
    (gJ,) = torch.autograd.grad(0.5 * torch.sum(wt * (q - dt) ** 2), q)
    plain = [fd.DirichletBC(W.sub(0), g0.detach()), bcs[1]]
    sens = adjoint.sensitivities(W, P, plain, p.detach(), gJ, spar.LINEAR_SOLVER_PARAMS, wrt_bcs=True)
    print(f"autograd: k1 {k1.grad.item():.6e} / {sens.k1:.6e}, k2 {k2.grad.item():.6e} / {sens.k2:.6e}, beta "
          f"{beta.grad.item():.6e} / {sens.beta:.6e}, mu {mu.grad.item():.2e} / {sens.mu:.2e}")
    assert (k1.grad.item(), k2.grad.item(), beta.grad.item(), mu.grad.item()) == (sens.k1, sens.k2, sens.beta, sens.mu)
    assert g0.grad.shape == (s.n,) and torch.equal(g0.grad, sens.bcs[0].torch())
    inner = np.setdiff1d(np.arange(s.n), FR.boundary_nodes(s))
    assert float(g0.grad[torch.as_tensor(inner, device="cuda")].abs().max()) == 0.0
    # and the numbers are the restatement's
    p0 = AR.forward(s, *params, g)
    ref = AR.sensitivities(s, *params, p0, AR.dJ_of(p0, w, d))
    et = max(abs(a - b) / sc for a, b, sc in zip(sens.terms, ref.terms, ref.abs_terms))
    eb = float(np.abs(g0.grad.cpu().numpy() - ref.bcs[:s.n]).max() / np.abs(ref.bcs).max())
    print(f"   against the restatement: terms {et:.2e}, boundary gradient {eb:.2e} (bar 1e-10)")
    assert et <= 1e-10 and eb <= 1e-10
    # floats instead of tensors: no gradient asked, none formed
    p2 = adjoint.solve_dpp_torch(W, 1.0, 0.01, 3.0, 2.0, plain, spar.LINEAR_SOLVER_PARAMS)
    assert not p2.requires_grad and torch.equal(p2, p.detach())


# ---- C ABI refusals ----------------------------------------------------------------------------------------------------
def test_c_abi_refusals(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    cfg, _ = solver.translate_options(GMRES_ILU_TIGHT)
    buf, buf2 = np.zeros(64), np.zeros(64)
    out = (C.c_double * 3)()
    dev, dev2 = torch.zeros(64, dtype=torch.float64, device="cuda"), torch.zeros(64, dtype=torch.float64, device="cuda")
    hp, hp2 = buf.ctypes.data_as(C.c_void_p), buf2.ctypes.data_as(C.c_void_p)
    dp, dp2 = C.c_void_p(dev.data_ptr()), C.c_void_p(dev2.data_ptr())
    lib = _ffi.lib

    def msg():
        return (lib.pph_last_error(ctx._h) or b"").decode()

    # before a mesh
    for name, call in {"pph_dpp_bilinear": lambda: lib.pph_dpp_bilinear(ctx._h, hp, hp2, out),
                       "pph_dpp_bilinear_device": lambda: lib.pph_dpp_bilinear_device(ctx._h, dp, dp2, out)}.items():
        assert call() == _ffi.PPH_ERR_INVALID and msg() == f"{name} before pph_mesh_build"
    solves = {"pph_solve_rhs": lambda a, b: lib.pph_solve_rhs(ctx._h, C.byref(cfg), a, b, None, None, 0),
              "pph_solve_rhs_device": lambda a, b: lib.pph_solve_rhs_device(ctx._h, C.byref(cfg), a, b, None, None, 0)}
    for name, call in solves.items():
        a, b = (hp, hp2) if name == "pph_solve_rhs" else (dp, dp2)
        assert call(a, b) == _ffi.PPH_ERR_INVALID and msg() == "pph_solve_rhs before pph_assemble_dpp"
    # a mesh, no assembly: the bilinear forms work, the solves are refused
    ctx.mesh_build(2, _ffi.CELL_QUAD, 2, 2)
    for name, call in solves.items():
        a, b = (hp, hp2) if name == "pph_solve_rhs" else (dp, dp2)
        assert call(a, b) == _ffi.PPH_ERR_INVALID and msg() == "pph_solve_rhs before pph_assemble_dpp"
    ones = np.concatenate([np.ones(9), np.zeros(9)])
    assert ctx.dpp_bilinear(ones, ones) == (0.0, 0.0, pytest.approx(1.0, abs=1e-15))
    # NULL buffers
    assert lib.pph_dpp_bilinear(ctx._h, None, hp, out) == _ffi.PPH_ERR_INVALID and "NULL buffer" in msg()
    assert lib.pph_dpp_bilinear_device(ctx._h, dp, None, out) == _ffi.PPH_ERR_INVALID and "NULL buffer" in msg()
    assert lib.pph_dpp_bilinear_device(ctx._h, dp, dp2, None) == _ffi.PPH_ERR_INVALID and "NULL buffer" in msg()
    bnd = np.array([0, 1, 2, 3, 5, 6, 7, 8], dtype=np.int64)
    ctx.set_dirichlet(0, bnd, np.ones(8))
    ctx.set_dirichlet(1, bnd, np.zeros(8))
    ctx.assemble(1.0, 0.01, 1.0, 1.0, monolithic=True)
    for name, call in solves.items():
        a = hp if name == "pph_solve_rhs" else dp
        assert call(None, a) == _ffi.PPH_ERR_INVALID and "NULL buffer" in msg()
        assert call(a, None) == _ffi.PPH_ERR_INVALID and "NULL buffer" in msg()
        assert call(a, a) == _ffi.PPH_ERR_INVALID and "different buffers" in msg()
    assert lib.pph_solve_rhs_device(ctx._h, None, dp, dp2, None, None, 0) == _ffi.PPH_ERR_INVALID and "cfg is NULL" in msg()
    # and the call works: one free node
    b = np.zeros(18)
    b[4], b[13] = 1.0, 2.0
    x, info, _ = ctx.solve_rhs(cfg, b)
    s = FR.space(FR.QUAD, 1, 2, 2, 0)
    want = AR.solve_free(s, 1.0, 0.01, 1.0, 1.0, b)
    assert info.converged == 1 and np.abs(x - want).max() <= 1e-10 * np.abs(want).max()


def test_c_abi_refuses_slab_contexts():
    """Two ranks over gloo, each with its slab of a distributed mesh (world = 2): the four entry points return
    PPH_ERR_INVALID with their message, and the Python functions refuse before a context is used
    (tools/adjoint_slab_check.py)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tools", "adjoint_slab_check.py")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0 and "world=2 adjoint refusals: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
