#!/usr/bin/env python3
"""Phases of one public-API call (solve_dpp_nonlinear, PICARD_MG_INEXACT_SOLVER_PARAMS, N^3 Q1 cube, manufactured
boundary data - the call bench.py's config.api times), with perf_counter on the host: boundary data, assembly, solve,
result handling (the device copy into a torch tensor and the Function around it), then the whole public call, the same
call followed by a first host access (vector()), and the step alone (ctx.solve(fetch=False) on the assembled system,
synchronised).  The remainder = public call - step.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=256)
ap.add_argument("--reps", type=int, default=3, help="timed repetitions of each measurement (the median is reported)")
ap.add_argument("--skip-vector", action="store_true", help="leave out the call followed by vector() (a copy trace then shows "
                                                           "no solution-sized device-to-host copy at all)")
args = ap.parse_args()

import perphil_amd as pa  # noqa: E402
from perphil_amd import _ffi, fd, solver_parameters as spar  # noqa: E402
from perphil_amd.manufactured_solutions import exact_expressions_3d  # noqa: E402
from perphil_amd.solver import _apply_bcs, translate_options  # noqa: E402

N = args.cells
params = pa.DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
opts = spar.PICARD_MG_INEXACT_SOLVER_PARAMS
mesh = fd.UnitCubeMesh(N, N, N, hexahedral=True)
V = fd.FunctionSpace(mesh, "CG", 1)
W = V * V
_, p1, _, p2 = exact_expressions_3d(mesh, params)
bcs = [fd.DirichletBC(W.sub(0), p1, "on_boundary"), fd.DirichletBC(W.sub(1), p2, "on_boundary")]
sol = pa.solve_dpp_nonlinear(W, params, bcs, solver_parameters=opts)     # warm-up: objects, allocations, first solve
ctx = mesh.context()


def med(xs):
    return sorted(xs)[len(xs) // 2]


def phases():
    t = [time.perf_counter()]
    cfg, _ = translate_options(opts, nonlinear=True)
    _apply_bcs(ctx, W, bcs)
    t.append(time.perf_counter())
    ctx.assemble(1.0, 0.01, 1.0, 1.0, monolithic=False)
    t.append(time.perf_counter())
    _, info, _ = ctx.solve(cfg, fetch=False)
    t.append(time.perf_counter())
    f = fd.Function(W, ctx.solution_tensor(), name="dpp_solution")
    ctx.timers()
    t.append(time.perf_counter())
    del f
    return [1e3 * (b - a) for a, b in zip(t, t[1:])]


rows = [phases() for _ in range(args.reps)]
names = ["bcs_ms", "assemble_enqueue_ms", "solve_ms", "result_ms"]
out = {"cells": N, "dofs": W.dim(), "shared_runtime": _ffi.shared_runtime(),
       "phases": {k: round(med([r[i] for r in rows]), 3) for i, k in enumerate(names)}}

walls, walls_host = [], []
for _ in range(args.reps):
    t0 = time.perf_counter()
    sol = pa.solve_dpp_nonlinear(W, params, bcs, solver_parameters=opts)
    walls.append(1e3 * (time.perf_counter() - t0))
    del sol
for _ in range(0 if args.skip_vector else args.reps):
    t0 = time.perf_counter()
    sol = pa.solve_dpp_nonlinear(W, params, bcs, solver_parameters=opts)
    sol.solution.vector()
    walls_host.append(1e3 * (time.perf_counter() - t0))
    del sol
cfg, _ = translate_options(opts, nonlinear=True)
steps = []
for _ in range(args.reps):
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.solve(cfg, fetch=False)
    ctx.synchronize()
    steps.append(1e3 * (time.perf_counter() - t0))
out["api_call_ms"] = round(med(walls), 3)
out["api_call_then_vector_ms"] = round(med(walls_host), 3) if walls_host else None
out["step_ms"] = round(med(steps), 3)
out["host_remainder_ms"] = round(med(walls) - med(steps), 3)
out["fetch_stats"] = dict(_ffi.fetch_stats)
out["what"] = ("phases of one solve_dpp_nonlinear call (PICARD_MG_INEXACT_SOLVER_PARAMS, manufactured boundary data), "
               "median of --reps; assemble is enqueued only (its device time lands in solve); step = ctx.solve on the "
               "assembled system; remainder = api call - step")
print(json.dumps(out), flush=True)
mesh.context().close()
