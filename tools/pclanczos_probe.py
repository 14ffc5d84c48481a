"""Preconditioned-Lanczos probe ("Preconditioned extremes"): kappa(B A), steps and ms per step of
pph_preconditioned_extremes next to the isolated product of the same operator (pph_spmv_bench) and the isolated application
of the same preconditioner (pph_pc_bench; scalar blocks only - the monolithic preconditioners have no bench entry), on a
hexahedral CG-1 mesh with homogeneous Dirichlet data on the whole boundary.

  python tools/pclanczos_probe.py [--cells 128] [--cases A11:jacobi A11:ilu A11:mg monolithic:pph_block2] [--reps 200]

Prints one JSON line.  The step time is device_ms / iterations of the second of two calls (an event pair around the start
vector, every step and the host's check every 16 steps; the preconditioner's set-up is outside and reported by the first)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from perphil_amd import _ffi  # noqa: E402

WHICH = {"monolithic": 0, "M": 2, "A11": 3, "A22": 4}
PCS = {"jacobi": _ffi.PC_JACOBI, "pph_block2": _ffi.PC_BLOCK2, "ilu": _ffi.PC_ILU, "mg": _ffi.PC_MG, "pph_pmg": _ffi.PC_PMG}


def main(cells, cases, reps, tol, max_it):
    out = {"probe": "pclanczos", "cells": cells, "tol": tol, "max_it": max_it, "cases": {}}
    with _ffi.Context(0) as ctx:
        ctx.mesh_build(3, _ffi.CELL_HEX, cells, cells, cells)
        X = ctx.coords()
        b = np.nonzero((X == 0.0).any(axis=1) | (np.abs(X - 1.0) < 1e-12).any(axis=1))[0]
        del X
        for f in (0, 1):
            ctx.set_dirichlet(f, b, np.zeros(len(b)))
        ctx.assemble(1.0, 0.01, 1.0, 1.0, monolithic=any(c.startswith("monolithic") for c in cases))
        out["nodes"] = ctx.n
        out["dict_operators"] = ctx.timers()["dict_operators"]
        for case in cases:
            op, pc = case.split(":")
            w = WHICH[op]
            r = ctx.preconditioned_extremes(w, PCS[pc], tol=tol, max_it=max_it)
            r2 = ctx.preconditioned_extremes(w, PCS[pc], tol=tol, max_it=max_it)
            product_ms = ctx.spmv_bench(w, reps)
            apply_ms = ctx.pc_bench(w - 3, PCS[pc], reps)["apply_ms"] if w in (3, 4) else None
            step_ms = r2["device_ms"] / r2["iterations"]
            out["cases"][case] = {
                "rows": (2 if w == 0 else 1) * ctx.n, "iterations": r["iterations"], "converged": r["converged"],
                "lambda_min": r["lambda_min"], "lambda_max": r["lambda_max"], "kappa": r["kappa"],
                "estimate_min": r["estimate_min"], "estimate_max": r["estimate_max"], "setup_ms": r["setup_ms"],
                "device_ms": [r["device_ms"], r2["device_ms"]], "ms_per_step": step_ms, "product_ms": product_ms,
                "apply_ms": apply_ms, "step_over_product_plus_apply": step_ms / (product_ms + apply_ms) if apply_ms is not None else None,
                "repeatable": r["lambda_min"] == r2["lambda_min"] and r["lambda_max"] == r2["lambda_max"]}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--cases", nargs="+", default=["A11:jacobi", "A11:ilu", "A11:mg", "monolithic:pph_block2"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--max-it", type=int, default=2000)
    a = ap.parse_args()
    main(a.cells, a.cases, a.reps, a.tol, a.max_it)
