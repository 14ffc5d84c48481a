#!/usr/bin/env python3
"""Timing of the adjoint pieces on one device ("Adjoint"): pph_dpp_bilinear_device against the composition that
gives the same three numbers without it (three pph_dpp_nodal_flux_device calls with unit coefficients plus torch dots, on
the stored CSR K and M), and adjoint_solve beside solve_dpp.  One JSON line per measurement.

    python tools/adjoint_probe.py [--sizes q1:128,q1:256,q2:64] [--reps 20] [--solve 128]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import perphil_amd as pa  # noqa: E402
from perphil_amd import _ffi, adjoint, fd, solver, solver_parameters as spar  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s (data sheet); the measured copy rate is about 6.3e12


def timed(fn, reps, warm=3):
    """Median and minimum wall time in ms of fn(), which ends in a device synchronisation."""
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t))


def probe_bilinear(deg, n, reps):
    mesh = fd.UnitCubeMesh(n, n, n, hexahedral=True, comm=fd.COMM_SELF)
    ctx = mesh.context(degree=deg) if deg != 1 else mesh.context()
    N = ctx.n
    gen = torch.Generator(device="cuda").manual_seed(1)
    lam = torch.randn(2 * N, dtype=torch.float64, device="cuda", generator=gen)
    p = torch.randn(2 * N, dtype=torch.float64, device="cuda", generator=gen)
    new_ms, new_min = timed(lambda: ctx.dpp_bilinear(lam, p), reps)
    new = ctx.dpp_bilinear(lam, p)
    nbytes = 4 * N * 8 + ctx.ncell * ctx.m * 4          # four fields and the dof map once
    free0 = torch.cuda.mem_get_info()[0]

    def composition():
        r = ctx.dpp_nodal_flux(p, 1.0, 0.0, 0.0, 1.0)
        o0 = torch.dot(lam[:N], r[:N])
        r = ctx.dpp_nodal_flux(p, 0.0, 1.0, 0.0, 1.0)
        o1 = torch.dot(lam[N:], r[N:])
        r = ctx.dpp_nodal_flux(p, 0.0, 0.0, 1.0, 1.0)
        o2 = torch.dot(lam[:N] - lam[N:], r[:N])
        return o0.item(), o1.item(), o2.item()

    t0 = time.perf_counter()
    old = composition()                                  # the first call integrates and stores K and M
    first_ms = (time.perf_counter() - t0) * 1e3
    held = free0 - torch.cuda.mem_get_info()[0]
    old_ms, old_min = timed(composition, reps)
    diff = max(abs(a - b) / max(abs(b), 1e-300) for a, b in zip(new, old))
    print(json.dumps({"what": "bilinear", "degree": deg, "n": n, "nodes": N, "new_ms": new_ms, "new_min_ms": new_min,
                      "algorithmic_bytes": nbytes, "GBps": nbytes / (new_ms * 1e-3) / 1e9,
                      "hbm_peak_fraction": nbytes / (new_ms * 1e-3) / HBM_PEAK,
                      "composition_ms": old_ms, "composition_min_ms": old_min, "composition_first_ms": first_ms,
                      "speedup": old_ms / new_ms, "csr_KM_bytes": 2 * 8 * ctx.nnzb,
                      "csr_KM_and_pattern_bytes": (2 * 8 + 4) * ctx.nnzb + 8 * (N + 1), "device_bytes_taken_by_first_call": held,
                      "relative_difference": diff}), flush=True)
    ctx.close()
    mesh._ctx = None
    mesh.__dict__.pop("_ctx_deg", None)


def probe_solve(n, reps):
    """adjoint_solve beside solve_dpp with the same options; the adjoint's right-hand side is the forward system's own
    lifted one, so both run the same iterations and the difference is the wrapper."""
    mesh = fd.UnitCubeMesh(n, n, n, hexahedral=True, comm=fd.COMM_SELF)
    V = fd.FunctionSpace(mesh, "CG", 1)
    W = V * V
    P = pa.DPPParameters()
    _, e1, _, e2 = pa.exact_expressions_3d(mesh, P)
    bcs = [fd.DirichletBC(W.sub(0), e1), fd.DirichletBC(W.sub(1), e2)]
    opts = spar.PICARD_MG_INEXACT_SOLVER_PARAMS
    fwd = []

    def forward():
        fwd.append(solver.solve_dpp_nonlinear(W, P, bcs, opts))
        torch.cuda.synchronize()

    f_ms, f_min = timed(forward, reps)
    ctx = mesh.context()
    rhs = torch.from_numpy(ctx.rhs()[0]).cuda()
    adj = []

    def backward():
        adj.append(adjoint.adjoint_solve(W, P, bcs, rhs, opts, nonlinear=True))
        torch.cuda.synchronize()

    a_ms, a_min = timed(backward, reps)
    cfg, _ = solver.translate_options(opts, nonlinear=True)
    raw_f = timed(lambda: ctx.solve(cfg, fetch=False), reps)
    x = torch.empty_like(rhs)
    info = _ffi.SolveInfo()
    import ctypes as C

    def raw_rhs():
        st = _ffi.lib.pph_solve_rhs_device(ctx._h, C.byref(cfg), C.c_void_p(rhs.data_ptr()), C.c_void_p(x.data_ptr()),
                                           C.byref(info), None, 0)
        assert st == 0

    raw_a = timed(raw_rhs, reps)
    print(json.dumps({"what": "solve", "n": n, "solve_dpp_ms": f_ms, "solve_dpp_min_ms": f_min, "adjoint_solve_ms": a_ms,
                      "adjoint_solve_min_ms": a_min, "ratio": a_ms / f_ms, "pph_solve_device_ms": raw_f[0],
                      "pph_solve_rhs_device_ms": raw_a[0], "raw_ratio": raw_a[0] / raw_f[0],
                      "forward_sweeps": fwd[-1].iteration_number, "adjoint_sweeps": adj[-1].iteration_number,
                      "vector_bytes": 16 * ctx.n}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="q1:128,q1:256,q2:64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--solve", type=int, default=128)
    a = ap.parse_args()
    _ffi.require_shared_runtime("tools/adjoint_probe.py")
    for item in [s for s in a.sizes.split(",") if s]:
        kind, n = item.split(":")
        probe_bilinear(2 if kind == "q2" else 1, int(n), a.reps)
    if a.solve > 0:
        probe_solve(a.solve, a.reps)


if __name__ == "__main__":
    main()
