#!/usr/bin/env python3
"""Error norms of a distributed, device-resident result (launched by torch.distributed.run; tests/test_device_results.py):
every rank solves on its slab through the public API, then l2_error / h1_seminorm_error run with Function.gather patched
to raise - each rank integrates over its owned cells on the device and the squares are summed over the ranks.  The
reference is the serial host path on the gathered field (afterwards): equal to 1e-12 relative.  Exit code 0 = agreement
on every rank."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, nargs=3, default=[12, 10, 16], metavar=("NX", "NY", "NZ"))
ap.add_argument("--kind", default="hex", choices=["hex", "tet"])
ap.add_argument("--backend", default="gloo")
args = ap.parse_args()

import perphil_amd as pa  # noqa: E402
from perphil_amd import fd, postprocessing as pp, solver_parameters as spar  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
dist.init_process_group(backend=args.backend)

nx, ny, nz = args.cells
params = pa.DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
mesh = fd.UnitCubeMesh(nx, ny, nz, hexahedral=(args.kind == "hex"))
V = fd.FunctionSpace(mesh, "CG", 1)
W = V * V
_, p1, _, p2 = pa.exact_expressions_3d(mesh, params)
sol = pa.solve_dpp_nonlinear(W, params, [fd.DirichletBC(W.sub(0), p1), fd.DirichletBC(W.sub(1), p2)],
                             solver_parameters=spar.PICARD_MG_SOLVER_PARAMS)
ok = mesh.distributed and sol.solution.on_device


def curve(X):
    return np.sin(X[:, 0]) * X[:, 1] + X[:, 2]


exact_here = [lambda f: (p1, p2)[f], lambda f: fd.Function(V).interpolate((p1, p2)[f]), lambda f: fd.Constant(0.5),
              lambda f: curve]


def refuse(self):
    raise AssertionError("Function.gather called by the norms")


real_gather = fd.Function.gather
fd.Function.gather = refuse
got = []
for f in (0, 1):
    for ex in exact_here:
        e = ex(f)
        got.append((pp.l2_error(sol.solution.sub(f), e), pp.h1_seminorm_error(sol.solution.sub(f), e)))
# the sampled path in many chunks (ranks make different numbers of calls; one ghost refresh, one sum over the ranks)
u0 = sol.solution.sub(0).torch()
got.append(mesh.context().error_norms_sampled_device(u0, curve, None, 6, chunk_cells=97 + 13 * rank))
ok = ok and sol.solution.on_device
fd.Function.gather = real_gather

# the serial host path on the same field, gathered afterwards
full = sol.gather().solution
twin = full.function_space().mesh()
Vt = fd.FunctionSpace(twin, "CG", 1)
exact_twin = [lambda f: (p1, p2)[f], lambda f: fd.Function(Vt).interpolate((p1, p2)[f]), lambda f: fd.Constant(0.5),
              lambda f: curve]
want = []
for f in (0, 1):
    for ex in exact_twin:
        e = ex(f)
        want.append((pp.l2_error(full.sub(f), e), pp.h1_seminorm_error(full.sub(f), e)))
want.append(want[3])
for (a, b), (c, d) in zip(got, want):
    if not (abs(a - c) <= 1e-12 * abs(c) and abs(b - d) <= 1e-12 * abs(d)):
        print(f"rank {rank}: device ({a!r}, {b!r}) vs serial ({c!r}, {d!r})", flush=True)
        ok = False
if ok:
    print(f"rank {rank}: device norms ok ({len(got)} pairs, world {world})", flush=True)
dist.destroy_process_group()
sys.exit(0 if ok else 1)
