"""Per-step time of a transient run with wells and a distributed source against the same run without sources (DESIGN.md,
"Wells and sources: measured"): hexahedral CG-1 mesh, CG + pph_cmg, backward Euler, homogeneous Dirichlet data on the whole
boundary, a device-resident random initial field.

  python tools/transient_sources_probe.py [--cells 128] [--steps 20] [--wells 64] [--sources 1] [--package-root DIR]

--sources 0 uses nothing but the entry points a library without sources has (pph_transient_steps_device), so the same script
times an older build: --package-root names the directory that holds that build's perphil_amd package.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--wells", type=int, default=64)
    ap.add_argument("--sources", type=int, default=1)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    import torch

    from perphil_amd import fd, solver, solver_parameters as spar

    n1 = a.cells
    mesh = fd.Mesh(3, fd.CELL_HEX, n1, n1, n1, comm=fd.COMM_SELF)
    ctx = mesh.context()
    n = ctx.n
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randn(2 * n, dtype=torch.float64, device="cuda", generator=g)
    idx = torch.arange(n, device="cuda")
    px = n1 + 1
    i, j, k = idx % px, (idx // px) % px, idx // (px * px)
    nodes = idx[(i == 0) | (i == n1) | (j == 0) | (j == n1) | (k == 0) | (k == n1)]
    for f in (0, 1):
        ctx.set_dirichlet_device(f, nodes, torch.zeros(nodes.numel(), dtype=torch.float64, device="cuda"))
    k1, k2, beta, mu, S, dt = 1.0, 0.01, 1.0, 1.0, (1.0, 20.0), 1e-3
    cfg, _ = solver.translate_options(spar.CG_CMG_PARAMS)
    out = {"probe": "transient_sources", "cells": n1, "nodes": n, "steps": a.steps, "sources": a.sources, "wells": a.wells}
    rng = np.random.default_rng(3)
    coef = None
    if a.sources:
        z = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
        z[:n] = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
        r = ctx.dpp_nodal_flux(z, 0.0, 0.0, 1.0, 1.0)                        # (M f, -M f)
        ctx.set_option("invalidate_KM", 1)
        dense = torch.zeros((1, 2 * n), dtype=torch.float64, device="cuda")
        dense[0, :n] = r[:n]
        pts = torch.from_numpy(rng.random((a.wells, 3))).cuda()
        t0 = time.perf_counter()
        outside = ctx.sources_set(dense, pts, (np.arange(a.wells) % 2).astype(np.int32))
        out["sources_set_ms"] = (time.perf_counter() - t0) * 1e3
        out["outside"] = outside
        coef = rng.standard_normal((a.steps, 1 + a.wells))
        b = torch.randn(2 * n, dtype=torch.float64, device="cuda", generator=g)
        ctx.sources_apply(coef[0], b)
        torch.cuda.synchronize()
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            ctx.sources_apply(coef[0], b)                                    # upload of one row, two kernels, synchronise
            ts.append((time.perf_counter() - t0) * 1e3)
        out["sources_apply_call_ms_median"] = float(np.median(ts))
    ctx.transient_begin(k1, k2, beta, mu, S, 1.0, dt, monolithic=True)
    kw = {} if coef is None else {"coef": coef[:2]}
    q = p.clone()
    ctx.transient_steps(cfg, q, 2, **kw)                                     # warm-up: hierarchy, dictionaries
    per_step = []
    for rep in range(3):
        q = p.clone()
        kw = {} if coef is None else {"coef": coef}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done, infos, norms = ctx.transient_steps(cfg, q, a.steps, **kw)
        torch.cuda.synchronize()
        per_step.append((time.perf_counter() - t0) * 1e3 / a.steps)
    out["ms_per_step"] = per_step
    out["ms_per_step_median"] = float(np.median(per_step))
    out["iterations"] = [int(x.iterations) for x in infos]
    out["ms_per_iteration_median"] = out["ms_per_step_median"] * a.steps / max(1, sum(out["iterations"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
