#!/usr/bin/env python3
"""Adjoint entry points on a distributed mesh (launched by torch.distributed.run, gloo): every rank holds a slab context
(world > 1), on which the four C entry points of pph_adjoint.hip return PPH_ERR_INVALID with their message - they run on
whole meshes only - and the Python functions refuse, naming comm=fd.COMM_SELF, before they use a context.  Exit code 0 =
every rank saw the refusals."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from perphil_amd import DPPParameters, _ffi, adjoint, fd, solver  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
dist.init_process_group(backend="gloo")

mesh = fd.UnitCubeMesh(3, 4, 6, hexahedral=True)
ctx = mesh.context()
ok = mesh.distributed
n = mesh.num_local_vertices()
V = fd.FunctionSpace(mesh, "CG", 1)
W = V * V
bcs = [fd.DirichletBC(W.sub(0), 1.0), fd.DirichletBC(W.sub(1), 0.0)]
P = DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
opts = {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-8}
cfg, _ = solver.translate_options(opts)
solver._apply_bcs(ctx, W, bcs)
ctx.assemble(1.0, 0.01, 1.0, 1.0, monolithic=True)      # (the solves are refused for the slab, not for a missing system)

host, host2 = np.zeros(2 * n), np.zeros(2 * n)
dev = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
dev2 = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
out = (C.c_double * 3)()
hp, hp2 = host.ctypes.data_as(C.c_void_p), host2.ctypes.data_as(C.c_void_p)
dp, dp2 = C.c_void_p(dev.data_ptr()), C.c_void_p(dev2.data_ptr())
lib = _ffi.lib
calls = {"pph_dpp_bilinear": (lambda: lib.pph_dpp_bilinear(ctx._h, hp, hp2, out), "pph_dpp_bilinear"),
         "pph_dpp_bilinear_device": (lambda: lib.pph_dpp_bilinear_device(ctx._h, dp, dp2, out), "pph_dpp_bilinear_device"),
         "pph_solve_rhs": (lambda: lib.pph_solve_rhs(ctx._h, C.byref(cfg), hp, hp2, None, None, 0), "pph_solve_rhs"),
         "pph_solve_rhs_device": (lambda: lib.pph_solve_rhs_device(ctx._h, C.byref(cfg), dp, dp2, None, None, 0),
                                  "pph_solve_rhs")}
for name, (call, who) in calls.items():
    st = call()
    msg = (lib.pph_last_error(ctx._h) or b"").decode()
    if st != _ffi.PPH_ERR_INVALID or msg != f"{who} is implemented for single-context meshes":
        print(f"rank {rank}: {name} returned {st} ({msg!r})", flush=True)
        ok = False

# the Python functions
for call in (lambda: adjoint.adjoint_solve(W, P, bcs, host, opts),
             lambda: adjoint.sensitivities(W, P, bcs, host, host2, opts),
             lambda: adjoint.solve_dpp_torch(W, 1.0, 0.01, 1.0, 1.0, bcs, opts)):
    try:
        call()
        ok = False
        print(f"rank {rank}: a Python function accepted a distributed mesh", flush=True)
    except NotImplementedError as e:
        ok = ok and "comm=fd.COMM_SELF" in str(e)

flag = torch.tensor([1.0 if ok else 0.0])
dist.all_reduce(flag, op=dist.ReduceOp.MIN)
if rank == 0:
    print(f"world={world} adjoint refusals: {'ok' if flag.item() == 1.0 else 'FAILED'}", flush=True)
dist.barrier()
ctx.close()
dist.destroy_process_group()
sys.exit(0 if flag.item() == 1.0 else 1)
