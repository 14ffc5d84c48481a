"""Mass balance probe ("Mass balance"): the three device calls of pph_flux.hip on a hexahedral CG-1 mesh with a
device-resident random two-field function.

  python tools/mass_balance_probe.py [--cells 256] [--reps 20]

Every call is bracketed by a HIP event pair on the context stream (the host results' read-back and the final stream
synchronisation of a call are inside the bracket); the first nodal-flux call, which integrates K and M and builds the CSR
pattern, is timed apart.  Prints one JSON line with the medians and the algorithmic bytes of each kernel.  Under
`rocprofv3 --kernel-trace --stats` the per-dispatch durations of k_face_flux / k_integrate / k_dpp_nodal_flux are the kernel
times."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from perphil_amd import fd  # noqa: E402


def timed(ctx, fn):
    st = ctx.torch_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def main(cells, reps):
    n = cells
    mesh = fd.Mesh(3, fd.CELL_HEX, n, n, n, comm=fd.COMM_SELF)
    ctx = mesh.context()
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randn(2 * ctx.n, dtype=torch.float64, device="cuda", generator=g)
    p1 = p[:ctx.n]
    torch.cuda.synchronize()
    first = timed(ctx, lambda: ctx.dpp_nodal_flux(p, 1.0, 0.01, 1.0, 1.0))
    calls = {"boundary_flux": lambda: ctx.boundary_flux(p1, 1.0), "integrate": lambda: ctx.integrate(p1),
             "dpp_nodal_flux": lambda: ctx.dpp_nodal_flux(p, 1.0, 0.01, 1.0, 1.0)}
    ms = {}
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        t = [timed(ctx, fn) for _ in range(reps)]
        ms[name] = {"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t)}
    boxes = 6 * n * n
    bytes_ = {"boundary_flux": boxes * (8 * 4 + 8 * 8),                    # dof map + nodal values of the boundary boxes (no coordinates are read)
              "integrate": n ** 3 * 8 * 4 + 8 * ctx.n,                      # dof map of every cell + every nodal value once
              "dpp_nodal_flux": ctx.nnzb * (4 + 8 + 8) + ctx.n * (8 + 4 * 8)}  # col, K, M + row pointers, p (2n) in, r (2n) out
    print(json.dumps({"probe": "mass_balance", "cells": n, "nodes": ctx.n, "nnz": ctx.nnzb, "reps": reps,
                      "first_nodal_flux_call_ms": first, "calls": ms, "algorithmic_bytes": bytes_}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    main(a.cells, a.reps)
