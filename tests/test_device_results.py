"""Device-resident results: solve_dpp / solve_dpp_nonlinear leave the solution in GPU memory (a torch tensor of the
caching allocator), post-processing reads it there, and the host sees it on first access only - with the values the host
path gives, bit for bit."""
import gc
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import perphil_amd as pa
from perphil_amd import _ffi, fd, postprocessing as pp, solver_parameters as spar
from perphil_amd.solver import translate_options

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = pa.DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
CASES = {"hex32": (3, fd.CELL_HEX, 32, 32, 32), "tri2d": (2, fd.CELL_TRI, 24, 20, 0)}
SOLVES = {"nonlinear": (pa.solve_dpp_nonlinear, spar.PICARD_MG_SOLVER_PARAMS, True),
          "linear": (pa.solve_dpp, spar.FIELDSPLIT_MG_PARAMS, False)}


def _problem(case, params=PARAMS):
    dim, kind, nx, ny, nz = CASES[case]
    if dim == 2:
        mesh = fd.UnitSquareMesh(nx, ny, quadrilateral=(kind == fd.CELL_QUAD))
        _, p1, _, p2 = pa.exact_expressions(mesh, params)
    else:
        mesh = fd.UnitCubeMesh(nx, ny, nz, hexahedral=(kind == fd.CELL_HEX))
        _, p1, _, p2 = pa.exact_expressions_3d(mesh, params)
    V = fd.FunctionSpace(mesh, "CG", 1)
    return mesh, V, V * V, p1, p2


def _reference(case, opts, nonlinear, v1, v2, params=PARAMS):
    """ctx.solve(cfg, fetch=True) on a fresh context with the same problem (host boundary values v1 / v2)."""
    dim, kind, nx, ny, nz = CASES[case]
    cfg, _ = translate_options(opts, nonlinear=nonlinear)
    mesh = fd.Mesh(dim, kind, nx, ny, nz, comm=fd.COMM_SELF)
    nodes = mesh.boundary_nodes()
    with _ffi.Context(0) as ctx:
        ctx.mesh_build(dim, kind, nx, ny, nz)
        ctx.set_dirichlet(0, nodes, v1)
        ctx.set_dirichlet(1, nodes, v2)
        ctx.assemble(float(params.k1), float(params.k2), float(params.beta), float(params.mu), monolithic=not cfg.picard)
        x, _, _ = ctx.solve(cfg, fetch=True)
        return x.copy()


def _boundary_values(mesh, p1, p2):
    nodes = mesh.boundary_nodes()
    X = mesh.node_coordinates(nodes)
    return p1(X), p2(X)


@pytest.mark.parametrize("case", ["hex32", "tri2d"])
@pytest.mark.parametrize("kind", ["nonlinear", "linear"])
def test_solution_is_device_resident_and_bitwise_equal(case, kind):
    solve, opts, nonlinear = SOLVES[kind]
    mesh, V, W, p1, p2 = _problem(case)
    sol = solve(W, PARAMS, [fd.DirichletBC(W.sub(0), p1, "on_boundary"), fd.DirichletBC(W.sub(1), p2, "on_boundary")],
                solver_parameters=opts)
    assert sol.solution.on_device and all(f.on_device for f in sol.solution.split())
    ref = _reference(case, opts, nonlinear, *_boundary_values(mesh, p1, p2))
    got = sol.solution.vector()
    assert not sol.solution.on_device
    np.testing.assert_array_equal(got, ref)
    mesh.context().close()


def test_postprocessing_moves_no_solution_bytes():
    mesh, V, W, p1, p2 = _problem("hex32")
    sol = pa.solve_dpp_nonlinear(W, PARAMS, [fd.DirichletBC(W.sub(0), p1), fd.DirichletBC(W.sub(1), p2)],
                                 solver_parameters=spar.PICARD_MG_SOLVER_PARAMS)
    p1x = fd.Function(V).interpolate(p1)           # a host Function as the exact field
    exacts = [lambda f: (p1, p2)[f], lambda f: p1x, lambda f: fd.Constant(0.5),
              lambda f: (lambda X: np.sin(X[:, 0]) * X[:, 1])]
    before = dict(_ffi.fetch_stats)
    dev = []
    for f in (0, 1):
        for ex in exacts:
            dev.append((pp.l2_error(sol.solution.sub(f), ex(f)), pp.h1_seminorm_error(sol.solution.sub(f), ex(f))))
    t = sol.solution.torch()
    assert t.is_cuda and sol.solution.on_device
    assert _ffi.fetch_stats == before, "a solution-sized copy reached the host"
    sol.solution.vector()                          # materialise: the host path from here on
    assert _ffi.fetch_stats["fetches"] == before["fetches"] + 1
    host = []
    for f in (0, 1):
        for ex in exacts:
            host.append((pp.l2_error(sol.solution.sub(f), ex(f)), pp.h1_seminorm_error(sol.solution.sub(f), ex(f))))
    assert dev == host                              # bitwise
    assert all(v[0] > 0 for v in dev)
    mesh.context().close()


def test_kept_results_survive_later_solves_and_close():
    mesh, V, W, p1, p2 = _problem("hex32")
    opts = spar.PICARD_MG_SOLVER_PARAMS
    kept = []
    for k2, c in ((0.01, None), (0.01, 2.5), (0.05, 2.5)):
        params = pa.DPPParameters(k1=1.0, k2=k2, beta=1.0, mu=1.0)
        _, q1, _, q2 = pa.exact_expressions_3d(mesh, params)
        bc0 = q1 if c is None else fd.Constant(c)
        sol = pa.solve_dpp_nonlinear(W, params, [fd.DirichletBC(W.sub(0), bc0), fd.DirichletBC(W.sub(1), q2)],
                                     solver_parameters=opts)
        v1, v2 = _boundary_values(mesh, q1, q2)
        if c is not None:
            v1 = np.full_like(v1, c)
        kept.append((sol, params, v1, v2))
    mesh.context().close()
    for sol, params, v1, v2 in kept:
        assert sol.solution.on_device
        ref = _reference("hex32", opts, True, v1, v2, params)
        np.testing.assert_array_equal(sol.solution.vector(), ref)


def test_torch_view_data_ptr_and_stream_order():
    mesh, V, W, p1, p2 = _problem("hex32")
    sol = pa.solve_dpp_nonlinear(W, PARAMS, [fd.DirichletBC(W.sub(0), p1), fd.DirichletBC(W.sub(1), p2)],
                                 solver_parameters=spar.PICARD_MG_SOLVER_PARAMS)
    t = sol.solution.torch()
    # launched at once on torch's (default) stream: ordered after the library's copy by the stream contract
    snap, amax, s = t.clone(), t.abs().max(), t.sum()
    assert t.is_cuda and t.dtype == torch.float64 and sol.solution.torch().data_ptr() == t.data_ptr()
    n = V.dim()
    a, b = sol.solution.sub(0).torch(), sol.solution.sub(1).torch()
    assert a.data_ptr() == t.data_ptr() and b.data_ptr() == t.data_ptr() + 8 * n and a.shape == b.shape == (n,)
    host = sol.solution.vector()
    np.testing.assert_array_equal(snap.cpu().numpy(), host)
    assert amax.item() == np.abs(host).max()
    assert s.item() == pytest.approx(host.sum(), rel=1e-12)
    mesh.context().close()


@pytest.mark.parametrize("case", ["hex32", "tri2d"])
def test_device_boundary_data_give_the_same_solution(case):
    mesh, V, W, p1, p2 = _problem(case)
    opts = spar.PICARD_MG_SOLVER_PARAMS
    X = mesh.node_coordinates()
    g1, g2 = p1(X), p2(X)
    ref = pa.solve_dpp_nonlinear(W, PARAMS, [fd.DirichletBC(W.sub(0), g1), fd.DirichletBC(W.sub(1), g2)],
                                 solver_parameters=opts).solution.vector().copy()
    dev = torch.device("cuda", 0)
    f2 = fd.Function(V, torch.from_numpy(g2).to(dev))
    assert f2.on_device
    bcs = [fd.DirichletBC(W.sub(0), torch.from_numpy(g1).to(dev)), fd.DirichletBC(W.sub(1), f2)]
    nodes, vals = bcs[0].nodes_and_values()
    assert nodes.is_cuda and vals.is_cuda
    sol = pa.solve_dpp_nonlinear(W, PARAMS, bcs, solver_parameters=opts)
    assert f2.on_device                             # the boundary Function was read on the device
    np.testing.assert_array_equal(sol.solution.vector(), ref)
    ctx = mesh.context()
    applied = dict(ctx._bc_state)
    assert all(ctx.same_dirichlet(f, *bc.nodes_and_values()) for f, bc in enumerate(bcs))
    again = pa.solve_dpp_nonlinear(W, PARAMS, bcs, solver_parameters=opts)   # same device sets: not applied again
    assert all(ctx._bc_state[f] is applied[f] for f in (0, 1))
    np.testing.assert_array_equal(again.solution.vector(), ref)
    mesh.context().close()


def test_writes_after_materialisation_are_seen_by_the_norms():
    mesh, V, W, p1, p2 = _problem("hex32")
    sol = pa.solve_dpp_nonlinear(W, PARAMS, [fd.DirichletBC(W.sub(0), p1), fd.DirichletBC(W.sub(1), p2)],
                                 solver_parameters=spar.PICARD_MG_SOLVER_PARAMS)
    p = sol.solution.sub(0)
    before = pp.l2_error(p, fd.Constant(1.0)), pp.h1_seminorm_error(p, fd.Constant(1.0))
    g = np.cos(np.arange(W.dim(), dtype=np.float64))
    sol.solution.vector()[:] = g                    # (materialises: every view sees the host array from here on)
    assert not p.on_device
    after = pp.l2_error(p, fd.Constant(1.0)), pp.h1_seminorm_error(p, fd.Constant(1.0))
    plain = fd.Function(V, g[:V.dim()].copy())
    assert after == (pp.l2_error(plain, fd.Constant(1.0)), pp.h1_seminorm_error(plain, fd.Constant(1.0)))
    assert after != before
    mesh.context().close()


@pytest.mark.parametrize("case", ["hex32", "tri2d"])
def test_darcy_velocity_from_a_device_pressure(case):
    mesh, V, W, p1, p2 = _problem(case)
    sol = pa.solve_dpp_nonlinear(W, PARAMS, [fd.DirichletBC(W.sub(0), p1), fd.DirichletBC(W.sub(1), p2)],
                                 solver_parameters=spar.PICARD_MG_SOLVER_PARAMS)
    ph1, _ = pp.split_dpp_solution(sol.solution)
    assert ph1.on_device and sol.solution.on_device
    u_dev = pp.calculate_darcy_velocity_from_pressure(ph1, 1.0)
    assert u_dev.on_device
    u_host = pp.calculate_darcy_velocity_from_pressure(fd.Function(V, ph1.vector().copy()), 1.0)
    assert not u_host.on_device
    np.testing.assert_array_equal(u_dev.vector(), u_host.vector())
    mesh.context().close()


def test_deleting_kept_solutions_frees_their_memory():
    mesh, V, W, p1, p2 = _problem("hex32")
    bcs = [fd.DirichletBC(W.sub(0), p1), fd.DirichletBC(W.sub(1), p2)]
    gc.collect()                                    # (what earlier tests left behind goes first)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    kept = [pa.solve_dpp_nonlinear(W, PARAMS, bcs, solver_parameters=spar.PICARD_MG_SOLVER_PARAMS) for _ in range(3)]
    assert torch.cuda.memory_allocated() >= base + 3 * 8 * W.dim()
    del kept                                        # (no garbage collection: the last reference frees the memory)
    torch.cuda.synchronize()
    torch.empty(1, device="cuda:0")                 # (lets the allocator retire blocks whose stream uses have ended)
    assert torch.cuda.memory_allocated() == base
    mesh.context().close()


def test_separate_runtime_falls_back_to_host_results(monkeypatch):
    mesh, V, W, p1, p2 = _problem("tri2d")
    monkeypatch.setattr(_ffi, "_shared", False)
    sol = pa.solve_dpp_nonlinear(W, PARAMS, [fd.DirichletBC(W.sub(0), p1), fd.DirichletBC(W.sub(1), p2)],
                                 solver_parameters=spar.PICARD_MG_SOLVER_PARAMS)
    assert not sol.solution.on_device and isinstance(sol.solution.vector(), np.ndarray)
    with pytest.raises(RuntimeError, match="one HIP runtime"):
        fd.Function(V, torch.zeros(V.dim(), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(RuntimeError, match="one HIP runtime"):
        fd.DirichletBC(W.sub(0), torch.zeros(V.dim(), dtype=torch.float64, device="cuda:0")).nodes_and_values()
    mesh.context().close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,kind", [(2, "hex"), (4, "tet")])
def test_distributed_norms_without_gather(world, kind):
    """Ranks on one GPU over gloo: norms of a device-resident slab result equal the serial norms of the same field."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "device_norms_check.py"),
           "--kind", kind]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("device norms ok") == world
