#!/usr/bin/env python3
"""Mass balance on a distributed mesh (launched by torch.distributed.run, gloo): every rank holds a slab context
(world > 1), on which the six C entry points of pph_flux.hip return PPH_ERR_INVALID with their message - they run on whole
meshes only - while the public functions gather the field first (collective) and evaluate it on the serial twin, as
Function.at does.  Exit code 0 = every rank saw the refusals and the gathered results equal the COMM_SELF ones."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from perphil_amd import _ffi, fd, postprocessing as pp  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
dist.init_process_group(backend="gloo")

mesh = fd.UnitCubeMesh(3, 4, 6, hexahedral=True)
ctx = mesh.context()
ok = mesh.distributed
n = mesh.num_local_vertices()
host = np.zeros(2 * n)
dev = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
out = (C.c_double * 6)()
hp, dp = host.ctypes.data_as(C.c_void_p), C.c_void_p(dev.data_ptr())
calls = {"pph_integrate": lambda: _ffi.lib.pph_integrate(ctx._h, hp, out),
         "pph_integrate_device": lambda: _ffi.lib.pph_integrate_device(ctx._h, dp, out),
         "pph_boundary_flux": lambda: _ffi.lib.pph_boundary_flux(ctx._h, hp, 1.0, out),
         "pph_boundary_flux_device": lambda: _ffi.lib.pph_boundary_flux_device(ctx._h, dp, 1.0, out),
         "pph_dpp_nodal_flux": lambda: _ffi.lib.pph_dpp_nodal_flux(ctx._h, 1.0, 1.0, 1.0, 1.0, hp, hp),
         "pph_dpp_nodal_flux_device": lambda: _ffi.lib.pph_dpp_nodal_flux_device(ctx._h, 1.0, 1.0, 1.0, 1.0, dp, dp)}
for name, call in calls.items():
    st = call()
    msg = (_ffi.lib.pph_last_error(ctx._h) or b"").decode()
    if st != _ffi.PPH_ERR_INVALID or msg != f"{name} is implemented for single-context meshes":
        print(f"rank {rank}: {name} returned {st} ({msg!r})", flush=True)
        ok = False

# the public functions: gather, then the serial twin
V = fd.FunctionSpace(mesh, "CG", 1)
f = fd.Function(V).interpolate(lambda X: X[:, 0] ** 2 + 2.0 * X[:, 1] - 3.0 * X[:, 2] * X[:, 0])
twin = fd.UnitCubeMesh(3, 4, 6, hexahedral=True, comm=fd.COMM_SELF)
g = fd.Function(fd.FunctionSpace(twin, "CG", 1)).interpolate(lambda X: X[:, 0] ** 2 + 2.0 * X[:, 1] - 3.0 * X[:, 2] * X[:, 0])
ok = ok and pp.integrate(f) == pp.integrate(g) and pp.boundary_fluxes(f, 2.0) == pp.boundary_fluxes(g, 2.0)

flag = torch.tensor([1.0 if ok else 0.0])
dist.all_reduce(flag, op=dist.ReduceOp.MIN)
if rank == 0:
    print(f"world={world} mass balance refusals: {'ok' if flag.item() == 1.0 else 'FAILED'}", flush=True)
dist.barrier()
ctx.close()
dist.destroy_process_group()
sys.exit(0 if flag.item() == 1.0 else 1)
