#!/usr/bin/env python3
"""The transient entry points on a distributed mesh (launched by torch.distributed.run, gloo): every rank holds a slab context
(world > 1), on which pph_dpp_step_rhs*, pph_assemble_dpp_shifted with a sigma != 0, pph_transient_begin and
pph_transient_steps* return PPH_ERR_INVALID with their message - they run on whole meshes only - and solve_dpp_transient
raises NotImplementedError before it touches a context.  The context stays usable: the plain assembly still runs.
Exit code 0 = every rank saw the refusals."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import perphil_amd as pa  # noqa: E402
from perphil_amd import _ffi, fd, solver, solver_parameters as spar  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
dist.init_process_group(backend="gloo")

mesh = fd.UnitCubeMesh(3, 4, 6, hexahedral=True)
ctx = mesh.context()
ok = mesh.distributed
n = mesh.num_local_vertices()
host, out = np.zeros(2 * n), np.zeros(2 * n)
dev, dout = torch.zeros(2 * n, dtype=torch.float64, device="cuda"), torch.zeros(2 * n, dtype=torch.float64, device="cuda")
hp, op = host.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
dp, dop = C.c_void_p(dev.data_ptr()), C.c_void_p(dout.data_ptr())
cfg, _ = solver.translate_options(spar.CG_JACOBI_PARAMS)
done = C.c_int(0)
single = "is implemented for single-context meshes"
calls = {
    "pph_dpp_step_rhs": (lambda: _ffi.lib.pph_dpp_step_rhs(ctx._h, 1.0, 1.0, 1.0, 1.0, hp, op), f"pph_dpp_step_rhs {single}"),
    "pph_dpp_step_rhs_device": (lambda: _ffi.lib.pph_dpp_step_rhs_device(ctx._h, 1.0, 1.0, 1.0, 1.0, dp, dop),
                                f"pph_dpp_step_rhs_device {single}"),
    "pph_assemble_dpp_shifted": (lambda: _ffi.lib.pph_assemble_dpp_shifted(ctx._h, 1.0, 1.0, 1.0, 1.0, 2.0, 0.0, 0),
                                 "pph_assemble_dpp_shifted: per-field mass coefficients are implemented for single-context meshes"),
    "pph_transient_begin": (lambda: _ffi.lib.pph_transient_begin(ctx._h, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 0.1, 0),
                            f"pph_transient_begin {single}"),
    "pph_transient_steps": (lambda: _ffi.lib.pph_transient_steps(ctx._h, C.byref(cfg), hp, 1, 0.0, None, None, C.byref(done)),
                            f"pph_transient_steps {single}"),
    "pph_transient_steps_device": (lambda: _ffi.lib.pph_transient_steps_device(ctx._h, C.byref(cfg), dp, 1, 0.0, None, None,
                                                                               C.byref(done)), f"pph_transient_steps {single}"),
}
for name, (call, want) in calls.items():
    st = call()
    msg = (_ffi.lib.pph_last_error(ctx._h) or b"").decode()
    if st != _ffi.PPH_ERR_INVALID or msg != want:
        print(f"rank {rank}: {name} returned {st} ({msg!r})", flush=True)
        ok = False

# the public function refuses before a context is used
V = fd.FunctionSpace(mesh, "CG", 1)
W = V * V
bcs = [fd.DirichletBC(W.sub(0), 1.0), fd.DirichletBC(W.sub(1), 0.0)]
try:
    pa.solve_dpp_transient(W, pa.DPPParameters(), bcs, np.zeros(W.local_dim()), 0.1, 2, solver_parameters=spar.CG_JACOBI_PARAMS)
    ok = False
except NotImplementedError as e:
    ok = ok and "comm=fd.COMM_SELF" in str(e)

# ... and the context still works: the steady Picard solve of the slabs (collective)
sol = pa.solve_dpp_nonlinear(W, pa.DPPParameters(), bcs, solver_parameters=spar.PICARD_MG_SOLVER_PARAMS)
ok = ok and bool(sol.info.get("converged"))

flag = torch.tensor([1.0 if ok else 0.0])
dist.all_reduce(flag, op=dist.ReduceOp.MIN)
if rank == 0:
    print(f"world={world} transient refusals: {'ok' if flag.item() == 1.0 else 'FAILED'}", flush=True)
dist.barrier()
ctx.close()
dist.destroy_process_group()
sys.exit(0 if flag.item() == 1.0 else 1)
