#!/usr/bin/env python3
"""The entry points of the transient adjoint on a distributed mesh (launched by torch.distributed.run, gloo): every rank holds a
slab context (world > 1), on which pph_transient_bilinear*, pph_eval_points_adjoint*, pph_transient_steps_record* and
pph_transient_adjoint* return PPH_ERR_INVALID with their message - they run on whole meshes only.  The context stays usable:
the plain assembly and solve still run.  Exit code 0 = every rank saw the refusals."""
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
N = 2
host, traj, terms = np.zeros(2 * n), np.zeros((N + 1, 2 * n)), np.zeros((N, 5))
dev = torch.zeros((N + 1, 2 * n), dtype=torch.float64, device="cuda")
hp, tp, op = (a.ctypes.data_as(C.c_void_p) for a in (host, traj, terms))
dp = C.c_void_p(dev.data_ptr())
cfg, _ = solver.translate_options(spar.CG_JACOBI_PARAMS)
done, nout, out5 = C.c_int(0), C.c_int64(0), (C.c_double * 5)()
single = "is implemented for single-context meshes"
lib = _ffi.lib
calls = {
    "pph_transient_bilinear": (lambda: lib.pph_transient_bilinear(ctx._h, hp, hp, hp, 1.0, out5), f"pph_transient_bilinear {single}"),
    "pph_transient_bilinear_device": (lambda: lib.pph_transient_bilinear_device(ctx._h, dp, dp, dp, 1.0, out5),
                                      f"pph_transient_bilinear_device {single}"),
    "pph_eval_points_adjoint": (lambda: lib.pph_eval_points_adjoint(ctx._h, hp, 1, hp, 1, 1e-12, hp, C.byref(nout)),
                                f"point evaluation {single}"),
    "pph_eval_points_adjoint_device": (lambda: lib.pph_eval_points_adjoint_device(ctx._h, dp, 1, dp, 1, 1e-12, dp, C.byref(nout)),
                                       f"point evaluation {single}"),
    "pph_transient_steps_record": (lambda: lib.pph_transient_steps_record(ctx._h, C.byref(cfg), hp, 1, 0.0, None, None,
                                                                          C.byref(done), tp), f"pph_transient_steps {single}"),
    "pph_transient_steps_record_device": (lambda: lib.pph_transient_steps_record_device(ctx._h, C.byref(cfg), dp, 1, 0.0, None, None,
                                                                                        C.byref(done), dp),
                                          f"pph_transient_steps {single}"),
    "pph_transient_adjoint": (lambda: lib.pph_transient_adjoint(ctx._h, C.byref(cfg), tp, tp, None, 0, None, 1e-12, N, op, hp, None,
                                                                None, C.byref(done)), f"pph_transient_adjoint {single}"),
    "pph_transient_adjoint_device": (lambda: lib.pph_transient_adjoint_device(ctx._h, C.byref(cfg), dp, dp, None, 0, None, 1e-12, N,
                                                                              op, dp, None, None, C.byref(done)),
                                     f"pph_transient_adjoint {single}"),
}
for name, (call, want) in calls.items():
    st = call()
    msg = (lib.pph_last_error(ctx._h) or b"").decode()
    if st != _ffi.PPH_ERR_INVALID or msg != want:
        print(f"rank {rank}: {name} returned {st} ({msg!r})", flush=True)
        ok = False

# ... and the context still works: the steady Picard solve of the slabs (collective)
V = fd.FunctionSpace(mesh, "CG", 1)
W = V * V
bcs = [fd.DirichletBC(W.sub(0), 1.0), fd.DirichletBC(W.sub(1), 0.0)]
sol = pa.solve_dpp_nonlinear(W, pa.DPPParameters(), bcs, solver_parameters=spar.PICARD_MG_SOLVER_PARAMS)
ok = ok and bool(sol.info.get("converged"))

flag = torch.tensor([1.0 if ok else 0.0])
dist.all_reduce(flag, op=dist.ReduceOp.MIN)
if rank == 0:
    print(f"world={world} transient adjoint refusals: {'ok' if flag.item() == 1.0 else 'FAILED'}", flush=True)
dist.barrier()
ctx.close()
dist.destroy_process_group()
sys.exit(0 if flag.item() == 1.0 else 1)
