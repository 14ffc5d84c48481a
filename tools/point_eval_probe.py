"""Point evaluation probes ("Point evaluation").

  python tools/point_eval_probe.py kernel {hex1|hex2} {lattice|random} [--points 4194304] [--reps 20]
      repeated launches of the evaluation kernel on a 128^3 Q1 / 64^3 Q2 hexahedral field with points in lattice order
      (consecutive threads gather neighbouring cells) or uniformly random; meant to run under
      `rocprofv3 --kernel-trace --stats`, whose per-dispatch durations are the measurement.  Prints the wall time per call
      (stream synchronisation included) as a cross-check.
  python tools/point_eval_probe.py line [--cells 256] [--reps 20]
      Function.at on one line of cells + 1 points through a device-resident two-field solution, against the full host copy
      (vector()) plus indexing, the only way to read such a line without point evaluation."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from perphil_amd import fd  # noqa: E402


def kernel(which, order, m, reps):
    deg, n = (1, 128) if which == "hex1" else (2, 64)
    mesh = fd.Mesh(3, fd.CELL_HEX, n, n, n, comm=fd.COMM_SELF)
    ctx = mesh.context() if deg == 1 else mesh.context(degree=2)
    g = torch.Generator(device="cuda").manual_seed(1)
    u = torch.randn(ctx.n, dtype=torch.float64, device="cuda", generator=g)
    X = torch.rand((m, 3), dtype=torch.float64, device="cuda", generator=g)
    if order == "lattice":     # point i in box i * nbox / m, boxes in their own (x fastest) order; random inside the box
        box = (torch.arange(m, device="cuda", dtype=torch.int64) * (n ** 3)) // m
        c = torch.stack([box % n, (box // n) % n, box // (n * n)], dim=1).to(torch.float64)
        X = (c + X) / n
    for _ in range(3):
        ctx.eval_points_device(u, X)
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.eval_points_device(u, X)
        t.append(time.perf_counter() - t0)
    print(json.dumps({"probe": "kernel", "field": which, "order": order, "points": m, "nodes_per_cell": ctx.m,
                      "wall_ms_median_per_call": 1e3 * float(np.median(t)), "reps": reps}))


def line(cells, reps):
    mesh = fd.Mesh(3, fd.CELL_HEX, cells, cells, cells, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    mesh.context()
    X = np.stack([np.full(cells + 1, 0.5 + 0.25 / cells), np.full(cells + 1, 0.37), np.arange(cells + 1) / cells], axis=1)
    data = torch.randn(W.dim(), dtype=torch.float64, device="cuda")
    sol = fd.Function(W, data)
    for _ in range(3):
        sol.sub(0).at(X)
    t_at = []
    for _ in range(reps):
        t0 = time.perf_counter()
        sol.sub(0).at(X)
        t_at.append(time.perf_counter() - t0)
    assert sol.on_device
    px = cells + 1
    idx = (cells // 2) + px * ((cells // 2) + px * np.arange(px))
    t_copy = []
    for _ in range(4):
        f = fd.Function(W, data.clone())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vals = f.sub(0).vector()[idx]
        t_copy.append(time.perf_counter() - t0)
        assert not f.on_device and vals.shape == (px,)
    print(json.dumps({"probe": "line", "cells": cells, "points": cells + 1, "solution_bytes": 8 * W.dim(),
                      "at_ms_median": 1e3 * float(np.median(t_at)), "at_ms_min": 1e3 * min(t_at),
                      "host_copy_plus_index_ms": [1e3 * x for x in t_copy]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("probe", choices=["kernel", "line"])
    ap.add_argument("field", nargs="?", default="hex1", choices=["hex1", "hex2"])
    ap.add_argument("order", nargs="?", default="random", choices=["lattice", "random"])
    ap.add_argument("--points", type=int, default=1 << 22)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    kernel(a.field, a.order, a.points, a.reps) if a.probe == "kernel" else line(a.cells, a.reps)
