"""Mass balance on the device (pph_flux.hip through perphil_amd.postprocessing) against the NumPy restatement of
tests/flux_reference.py, on all four cell kinds and degrees 1 and 2.

Shapes: 5x3 / 3x4x2 (nx != ny != nz: an axis mix-up shows), 2x2 / 2x2x2 (every cell touches a corner), 1x3 (one cell touches
both x sides), 300x4 (a y side's 300 facets cross the 256 lanes of a workgroup, the launch has several workgroups) and
20x17x2 (340 / 680 facets per z side, every cell touches a z side).

Bars.  Closed forms: 1e-13 of kappa max|grad p| |side| (a few hundred terms of one rounding each).  Restatement: 1e-12 of
the sum of the absolute values of the terms added (integrals) or of the largest entry (r): the project's bar wherever only
the order of summation differs.  After a solve: 1e-10 of the same scales, the bar of the direct-equivalent path.
Every test prints its worst figure before it asserts."""
import ctypes as C
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import perphil_amd as pa  # noqa: E402
from perphil_amd import _ffi, fd, postprocessing as pp, solver_parameters as spar  # noqa: E402
import flux_reference as FR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES2, SHAPES3 = [(5, 3, 0), (2, 2, 0), (300, 4, 0), (1, 3, 0)], [(3, 4, 2), (2, 2, 2), (20, 17, 2)]
CASES = [(k, deg) + s for k in (FR.QUAD, FR.TRI, FR.HEX, FR.TET) for deg in (1, 2)
         for s in (SHAPES2 if k in (FR.QUAD, FR.TRI) else SHAPES3)]
IDS = [f"{('quad', 'tri', 'hex', 'tet')[c[0]]}{c[2]}x{c[3]}x{c[4]}-deg{c[1]}" for c in CASES]
K1, K2, BETA, MU, KAPPA = 1.0, 0.01, 3.0, 2.0, 2.5


class P:      # what the public functions read of DPPParameters
    k1, k2, beta, mu = K1, K2, BETA, MU


def _spaces(kind, deg, nx, ny, nz):
    mesh = fd.Mesh(FR.dim_of(kind), kind, nx, ny, nz, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(mesh, "CG", deg)
    return mesh, V, V * V


def _dev(space, u):
    return fd.Function(space, torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64).copy()).cuda())


@functools.lru_cache(maxsize=None)
def _random(case):
    """The random mixed field of a case, the restatement's figures and the device's, computed once and left unchanged."""
    kind, deg, nx, ny, nz = case
    s = FR.space(kind, deg, nx, ny, nz)
    p = np.random.default_rng(1000 + CASES.index(case)).standard_normal(2 * s.n)
    ref = {"I": FR.integrate(s, p[:s.n]), "I2": FR.integrate(s, p[s.n:]), "F": FR.boundary_fluxes(s, p[:s.n], KAPPA),
           "r": FR.nodal_fluxes(s, p, K1, K2, BETA, MU)}
    mesh, V, W = _spaces(kind, deg, nx, ny, nz)
    w = _dev(W, p)
    p1, p2 = w.subfunctions
    before = dict(_ffi.fetch_stats)
    gpu = []
    for _ in range(2):      # the second round is the determinism check's
        r = pp.consistent_fluxes(w, P)
        assert r.on_device and w.on_device and r.function_space() is W
        gpu.append({"I": pp.integrate(p1), "I2": pp.integrate(p2), "F": pp.boundary_fluxes(p1, KAPPA),
                    "T": pp.mass_transfer_rate(w, P), "r": r.torch().clone()})
    assert _ffi.fetch_stats == before      # nothing solution-sized went to the host
    for g in gpu:
        g["r"] = g["r"].cpu().numpy()
    return s, p, ref, gpu


def _grad_max(d):
    """max |grad p| over the unit box of the quadratic test field (|grad p|^2 is convex: attained at a corner)."""
    best = 0.0
    for c in range(1 << d):
        x, y, z = c & 1, (c >> 1) & 1, (c >> 2) & 1 if d == 3 else 0
        g = [2 * x + 2 * y - (z if d == 3 else 0), 2 * x - 6 * y] + ([2 * z - x] if d == 3 else [])
        best = max(best, float(np.linalg.norm(g)))
    return best


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_linear_fields_give_closed_form_fluxes_and_integral(case):
    kind, deg, nx, ny, nz = case
    mesh, V, _ = _spaces(kind, deg, nx, ny, nz)
    d = mesh.dim
    a, c = np.array([1.5, -2.0, 0.75])[:d], 0.3
    X = mesh.node_coordinates(degree=deg)
    f = _dev(V, X @ a + c)
    F = pp.boundary_fluxes(f, fd.Constant(KAPPA))
    assert sorted(F) == list(range(1, 2 * d + 1)) and f.on_device
    want = {s + 1: (KAPPA if s % 2 == 0 else -KAPPA) * a[s // 2] for s in range(2 * d)}
    err = max(abs(F[s] - want[s]) for s in F)
    tol = 1e-13 * KAPPA * float(np.linalg.norm(a))
    I = pp.integrate(f)
    print(f"linear {IDS[CASES.index(case)]}: flux error {err:.2e} (bar {tol:.2e}), integral error {abs(I - (a.sum() / 2 + c)):.2e}")
    assert err <= tol
    assert abs(I - (a.sum() / 2 + c)) <= 1e-13 * (np.abs(a).sum() + c)


@pytest.mark.parametrize("case", [c for c in CASES if c[1] == 2], ids=[i for c, i in zip(CASES, IDS) if c[1] == 2])
def test_quadratic_fields_give_closed_form_fluxes(case):
    """p = x^2 + 2xy - 3y^2 (+ z^2 - xz): grad p = (2x + 2y - z, 2x - 6y, 2z - x), linear, so a side integral is the value at
    the side's centre."""
    kind, deg, nx, ny, nz = case
    mesh, V, _ = _spaces(kind, deg, nx, ny, nz)
    d = mesh.dim
    X = mesh.node_coordinates(degree=deg)
    x, y = X[:, 0], X[:, 1]
    u = x * x + 2 * x * y - 3 * y * y
    h = 0.5 if d == 3 else 0.0      # (the z terms at a side's centre)
    want = {1: KAPPA * (1.0 - h), 2: -KAPPA * (3.0 - h), 3: KAPPA * 1.0, 4: KAPPA * 5.0}
    if d == 3:
        u = u + X[:, 2] ** 2 - x * X[:, 2]
        want.update({5: -KAPPA * 0.5, 6: -KAPPA * 1.5})
    F = pp.boundary_fluxes(_dev(V, u), KAPPA)
    err = max(abs(F[s] - want[s]) for s in want)
    tol = 1e-13 * KAPPA * _grad_max(d)
    print(f"quadratic {IDS[CASES.index(case)]}: flux error {err:.2e} (bar {tol:.2e})")
    assert sorted(F) == sorted(want) and err <= tol


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_fields_against_the_restatement(case):
    s, p, ref, gpu = _random(case)
    g = gpu[0]
    eI = max(abs(g["I"] - ref["I"][0]) / ref["I"][1], abs(g["I2"] - ref["I2"][0]) / ref["I2"][1])
    F, A = ref["F"]
    eF = max(abs(g["F"][k + 1] - F[k]) / A[k] for k in range(2 * s.dim))
    er = np.abs(g["r"] - ref["r"]).max() / np.abs(ref["r"]).max()
    print(f"random {IDS[CASES.index(case)]}: integral {eI:.2e}, fluxes {eF:.2e}, r {er:.2e} (bar 1e-12 each)")
    assert len(g["F"]) == 2 * s.dim and g["r"].shape == (2 * s.n,)
    assert eI <= 1e-12 and eF <= 1e-12 and er <= 1e-12


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_nodal_fluxes_sum_to_the_transfer(case):
    """1^T r1 = T = -1^T r2 on the device's own figures, for a field that solves nothing."""
    s, p, ref, gpu = _random(case)
    g = gpu[0]
    T = BETA / MU * (g["I"] - g["I2"])
    scale = BETA / MU * (ref["I"][1] + ref["I2"][1]) + np.abs(ref["r"]).sum()
    e1, e2 = abs(g["r"][:s.n].sum() - T), abs(g["r"][s.n:].sum() + T)
    print(f"identity {IDS[CASES.index(case)]}: {e1 / scale:.2e}, {e2 / scale:.2e} of the terms' absolute sum (bar 1e-12)")
    assert g["T"] == T and e1 <= 1e-12 * scale and e2 <= 1e-12 * scale


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_second_call_is_bitwise_equal(case):
    _, _, _, (a, b) = _random(case)
    assert a["I"] == b["I"] and a["I2"] == b["I2"] and a["F"] == b["F"] and a["T"] == b["T"]
    assert np.array_equal(a["r"], b["r"])


@pytest.mark.parametrize("case", [CASES[CASES.index((FR.HEX, 1, 3, 4, 2))], CASES[CASES.index((FR.TRI, 2, 300, 4, 0))]],
                         ids=["hex3x4x2-deg1", "tri300x4x0-deg2"])
def test_host_fields_give_the_same_bits(case):
    """Each kernel once more on a host-resident field (uploaded for the call)."""
    kind, deg, nx, ny, nz = case
    s, p, _, gpu = _random(case)
    _, _, W = _spaces(kind, deg, nx, ny, nz)
    w = fd.Function(W, p.copy())
    p1, p2 = w.subfunctions
    r = pp.consistent_fluxes(w, P)
    assert not r.on_device and not w.on_device
    assert pp.integrate(p1) == gpu[0]["I"] and pp.boundary_fluxes(p1, KAPPA) == gpu[0]["F"]
    assert np.array_equal(r.vector(), gpu[0]["r"])
    b = pp.mass_balance(w, P)
    assert b.transfer == gpu[0]["T"] and isinstance(b, pp.MassBalance)


def _solve(kind, deg, n, opts):
    params = pa.DPPParameters()
    d = FR.dim_of(kind)
    mesh = (fd.UnitSquareMesh(n, n, quadrilateral=True, comm=fd.COMM_SELF) if d == 2
            else fd.UnitCubeMesh(n, n, n, hexahedral=True, comm=fd.COMM_SELF))
    V = fd.FunctionSpace(mesh, "CG", deg)
    W = V * V
    _, e1, _, e2 = (pa.exact_expressions if d == 2 else pa.exact_expressions_3d)(mesh, params)
    sol = pa.solve_dpp(W, params, [fd.DirichletBC(W.sub(0), e1), fd.DirichletBC(W.sub(1), e2)], solver_parameters=opts)
    return params, sol.solution


GMRES_ILU_TIGHT = dict(spar.GMRES_ILU_PARAMS, ksp_rtol=1e-12)


@pytest.mark.parametrize("kind,deg,n", [(FR.QUAD, 1, 8), (FR.HEX, 1, 4), (FR.QUAD, 2, 8)], ids=["quad8-deg1", "hex4-deg1", "quad8-deg2"])
def test_mass_balance_of_a_solution(kind, deg, n):
    opts = spar.LINEAR_SOLVER_PARAMS if deg == 1 else GMRES_ILU_TIGHT
    params, sol = _solve(kind, deg, n, opts)
    b = pp.mass_balance(sol, params)
    s = FR.space(kind, deg, n, n, n if FR.dim_of(kind) == 3 else 0)
    x = sol.vector().copy()
    k1, k2, beta, mu = (float(v) for v in (params.k1, params.k2, params.beta, params.mu))
    ref = FR.mass_balance(s, x, k1, k2, beta, mu)
    (_, a1), (_, a2) = FR.integrate(s, x[:s.n]), FR.integrate(s, x[s.n:])
    bn = FR.boundary_nodes(s)
    figures = [("transfer", b.transfer, ref.transfer, beta / mu * (a1 + a2))]
    for f, kf in ((0, k1 / mu), (1, k2 / mu)):
        figures.append((f"outflow_consistent[{f}]", b.outflow_consistent[f], ref.outflow_consistent[f],
                        np.abs(ref.r[f * s.n + bn]).sum()))
        figures.append((f"imbalance[{f}]", b.imbalance[f], ref.imbalance[f], ref.scale))
        A = FR.boundary_fluxes(s, x[f * s.n:(f + 1) * s.n], kf)[1]
        for side in range(2 * s.dim):
            figures.append((f"outflow_direct[{f}][{side + 1}]", b.outflow_direct[f][side + 1], ref.outflow_direct[f][side], A[side]))
    worst = 0.0
    for name, got, want, scale in figures:
        e = abs(got - want) / scale
        worst = max(worst, e)
        print(f"{name}: {got:.15e} vs {want:.15e}: {e:.2e} of {scale:.3e}")
    assert worst <= 1e-10
    for f in (0, 1):
        bound = ref.interior_l1[f] + 1e-12 * ref.scale
        print(f"imbalance[{f}] = {b.imbalance[f]:.3e}, interior 1-norm of r = {ref.interior_l1[f]:.3e}, bound {bound:.3e}")
        assert abs(b.imbalance[f]) <= bound


def test_direct_and_consistent_outflows_differ_by_the_committed_gaps():
    """The gap between the two outflows is O(h) and carries no threshold: quadrilaterals 8x8, 16x16, 32x32, degree 1, equal
    the restatement's on the CPU's direct solve (tests/golden/mass_balance_gaps.json) to 1e-10 of the side fluxes' sum."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "mass_balance_gaps.json")))
    for n in (8, 16, 32):
        params, sol = _solve(FR.QUAD, 1, n, spar.LINEAR_SOLVER_PARAMS)
        b = pp.mass_balance(sol, params)
        for f in (0, 1):
            gap = sum(b.outflow_direct[f].values()) - b.outflow_consistent[f]
            scale = sum(abs(v) for v in b.outflow_direct[f].values()) + abs(b.outflow_consistent[f])
            print(f"{n}x{n} network {f + 1}: gap {gap:.12e}, committed {gold[str(n)][f]:.12e}, scale {scale:.3e}")
            assert abs(gap - gold[str(n)][f]) <= 1e-10 * scale


def test_c_abi_refuses_a_context_without_a_mesh(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    buf = np.zeros(16)
    out = (C.c_double * 6)()
    dev = torch.zeros(16, dtype=torch.float64, device="cuda")
    ptr, dptr = buf.ctypes.data_as(C.c_void_p), C.c_void_p(dev.data_ptr())
    calls = {"pph_integrate": lambda: _ffi.lib.pph_integrate(ctx._h, ptr, out),
             "pph_integrate_device": lambda: _ffi.lib.pph_integrate_device(ctx._h, dptr, out),
             "pph_boundary_flux": lambda: _ffi.lib.pph_boundary_flux(ctx._h, ptr, 1.0, out),
             "pph_boundary_flux_device": lambda: _ffi.lib.pph_boundary_flux_device(ctx._h, dptr, 1.0, out),
             "pph_dpp_nodal_flux": lambda: _ffi.lib.pph_dpp_nodal_flux(ctx._h, 1.0, 1.0, 1.0, 1.0, ptr, ptr),
             "pph_dpp_nodal_flux_device": lambda: _ffi.lib.pph_dpp_nodal_flux_device(ctx._h, 1.0, 1.0, 1.0, 1.0, dptr, dptr)}
    for name, call in calls.items():
        assert call() == _ffi.PPH_ERR_INVALID
        assert (_ffi.lib.pph_last_error(ctx._h) or b"").decode() == f"{name} before pph_mesh_build"
    ctx.mesh_build(2, _ffi.CELL_QUAD, 2, 2)
    assert _ffi.lib.pph_integrate(ctx._h, None, out) == _ffi.PPH_ERR_INVALID
    assert "NULL buffer" in (_ffi.lib.pph_last_error(ctx._h) or b"").decode()
    assert ctx.integrate(np.ones(9)) == pytest.approx(1.0, abs=1e-15)


def test_c_abi_refuses_slab_contexts():
    """Two ranks over gloo, each with its slab of a distributed mesh (world = 2): the six entry points return
    PPH_ERR_INVALID with their message, and the public functions gather first (tools/mass_balance_slab_check.py)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tools", "mass_balance_slab_check.py")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0 and "world=2 mass balance refusals: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
