"""Step right-hand side probe ("Transient: the step right-hand side"): b = -F A_unel p on a hexahedral CG-1 mesh with
a device-resident random two-field function, matrix-free (k_step_rhs, pph_transient.hip) and composed from the public pieces it
replaces (pph_dpp_nodal_flux_device on the stored K and M, then mask and sign as torch operations).

  python tools/transient_probe.py [--cells 128] [--reps 20] [--kind hex|tet] [--steps 10]

Every call is bracketed by a HIP event pair on the context stream (the call's final stream synchronisation is inside the
bracket).  The matrix-free path runs FIRST, before anything stores K or M, so that the device memory the composed path adds
shows.  Prints one JSON line with the medians, the algorithmic bytes per node and the device memory in use after each path.
Under `rocprofv3 --kernel-trace --stats` the per-dispatch durations of k_step_rhs / k_dpp_nodal_flux are the kernel times."""
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


def used_bytes():
    free, total = torch.cuda.mem_get_info()
    return total - free


def main(cells, reps, kind, steps=0):
    n = cells
    mesh = fd.Mesh(3, fd.CELL_HEX if kind == "hex" else fd.CELL_TET, n, n, n, comm=fd.COMM_SELF)
    ctx = mesh.context()
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randn(2 * ctx.n, dtype=torch.float64, device="cuda", generator=g)
    idx = torch.arange(ctx.n, device="cuda")
    px = n + 1
    i, j, k = idx % px, (idx // px) % px, idx // (px * px)
    con = (i == 0) | (i == n) | (j == 0) | (j == n) | (k == 0) | (k == n)
    nodes = idx[con]
    for f in (0, 1):
        ctx.set_dirichlet_device(f, nodes, torch.zeros(nodes.numel(), dtype=torch.float64, device="cuda"))
    con2 = torch.cat([con, con])
    torch.cuda.synchronize()
    args = (1.0, 0.01, 1.0, 1.0)

    def composed():
        r = ctx.dpp_nodal_flux(p, *args)
        return torch.where(con2, torch.zeros_like(r), -r)

    out = {"probe": "transient_step_rhs", "kind": kind, "cells": n, "nodes": ctx.n, "reps": reps}
    mem0 = used_bytes()
    for name, fn in (("step_rhs", lambda: ctx.step_rhs(p, *args)), ("composed", composed)):
        first = timed(ctx, fn)
        for _ in range(3):
            fn()
        t = [timed(ctx, fn) for _ in range(reps)]
        torch.cuda.synchronize()
        out[name] = {"first_call_ms": first, "median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t),
                     "device_bytes_added": used_bytes() - mem0}
    a, b = ctx.step_rhs(p, *args), composed()
    out["max_abs_difference"] = float((a - b).abs().max())
    out["max_abs_value"] = float(b.abs().max())
    # p (2 x 8 B) read once, the two masks, b (2 x 8 B) written once; the composed path: col, K, M per entry, row pointers, p, r
    out["algorithmic_bytes_per_node"] = {"step_rhs": 16 + 2 + 16,
                                         "dpp_nodal_flux": (ctx.nnzb * (4 + 8 + 8) + ctx.n * (8 + 4 * 8)) / ctx.n}
    for name, key in (("step_rhs", "step_rhs"), ("composed", "dpp_nodal_flux")):
        out[name]["algorithmic_GBps_at_median"] = out["algorithmic_bytes_per_node"][key] * ctx.n / out[name]["median_ms"] * 1e-6
    if steps > 0:
        out["stepping"] = stepping(ctx, p, steps)
    print(json.dumps(out))


def stepping(ctx, p, steps):
    """Per-step time of the fused loop (pph_transient_steps_device) and of the same step composed from the public pieces
    (dpp_nodal_flux + mask, solve_rhs, an axpy), backward Euler, under CG + pph_cmg and under the Picard-MG preset."""
    import time

    from perphil_amd import solver, solver_parameters as spar

    k1, k2, beta, mu, S, dt = 1.0, 0.01, 1.0, 1.0, (1.0, 20.0), 1e-3
    n = ctx.n
    out = {"steps": steps, "dt": dt, "storage": S}
    m0 = ctx_masks(ctx)
    for name, params, nonlinear in (("cg_cmg", spar.CG_CMG_PARAMS, False), ("picard_mg", spar.PICARD_MG_INEXACT_SOLVER_PARAMS, True)):
        cfg, _ = solver.translate_options(params, nonlinear=nonlinear)
        ctx.set_option("invalidate_KM", 1)               # (the composed steps below store K and M: the next assembly is the fused one again)
        ctx.transient_begin(k1, k2, beta, mu, S, 1.0, dt, monolithic=not cfg.picard)
        q = p.clone()
        ctx.transient_steps(cfg, q, 2)                      # warm-up: hierarchy, dictionaries, graphs
        q = p.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done, infos, norms = ctx.transient_steps(cfg, q, steps)
        torch.cuda.synchronize()
        fused = (time.perf_counter() - t0) * 1e3 / steps
        r = p.clone()
        r[m0] = 0.0

        def composed_step():
            b = -ctx.dpp_nodal_flux(r, k1, k2, beta, mu)
            b[m0] = 0.0
            d, info, _ = ctx.solve_rhs(cfg, b)
            r.add_(d)
            return info

        composed_step(); composed_step()
        r = p.clone()
        r[m0] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        its = [composed_step().iterations for _ in range(steps)]
        torch.cuda.synchronize()
        comp = (time.perf_counter() - t0) * 1e3 / steps
        out[name] = {"fused_ms_per_step": fused, "composed_ms_per_step": comp, "iterations_fused": [int(i.iterations) for i in infos],
                     "iterations_composed": [int(i) for i in its],
                     "max_abs_difference_of_the_final_fields": float((q - r).abs().max()), "max_abs_value": float(q.abs().max())}
    return out


def ctx_masks(ctx):
    """Boolean tensor [2n]: the dofs the probe's Dirichlet sets (whole boundary, both fields) constrain."""
    n1 = round(ctx.n ** (1.0 / 3.0))
    idx = torch.arange(ctx.n, device="cuda")
    i, j, k = idx % n1, (idx // n1) % n1, idx // (n1 * n1)
    con = (i == 0) | (i == n1 - 1) | (j == 0) | (j == n1 - 1) | (k == 0) | (k == n1 - 1)
    return torch.cat([con, con])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kind", default="hex", choices=("hex", "tet"))
    ap.add_argument("--steps", type=int, default=0, help="> 0: also time this many backward-Euler steps, fused and composed")
    a = ap.parse_args()
    main(a.cells, a.reps, a.kind, a.steps)
