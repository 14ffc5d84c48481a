"""Lanczos probe ("Extreme eigenvalues"): ms per Lanczos step of pph_extreme_eigenvalues next to the isolated
product of the same operator (pph_spmv_bench), on a hexahedral CG-1 mesh with homogeneous Dirichlet data on the whole boundary.

  python tools/lanczos_probe.py [--cells 128] [--which 3 0] [--reps 200]

Prints one JSON line.  The step time is device_ms / iterations of one call (an event pair around the whole call: the start
vector, every step, and the host's check every 32 steps are inside)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from perphil_amd import _ffi  # noqa: E402

NAMES = {0: "monolithic", 2: "M", 3: "A11", 4: "A22"}


def main(cells, which, reps):
    out = {"probe": "lanczos", "cells": cells, "operators": {}}
    with _ffi.Context(0) as ctx:
        ctx.mesh_build(3, _ffi.CELL_HEX, cells, cells, cells)
        X = ctx.coords()
        b = np.nonzero((X == 0.0).any(axis=1) | (np.abs(X - 1.0) < 1e-12).any(axis=1))[0]
        del X
        for f in (0, 1):
            ctx.set_dirichlet(f, b, np.zeros(len(b)))
        ctx.assemble(1.0, 0.01, 1.0, 1.0, monolithic=0 in which)
        out["nodes"] = ctx.n
        out["dict_operators"] = ctx.timers()["dict_operators"]
        for w in which:
            r = ctx.extreme_eigenvalues(w)
            r2 = ctx.extreme_eigenvalues(w)
            product_ms = ctx.spmv_bench(w, reps)
            out["operators"][NAMES[w]] = {
                "rows": (2 if w == 0 else 1) * ctx.n, "iterations": r["iterations"], "converged": r["converged"],
                "lambda_min": r["lambda_min"], "lambda_max": r["lambda_max"], "kappa": r["lambda_max"] / r["lambda_min"],
                "device_ms": [r["device_ms"], r2["device_ms"]], "ms_per_step": r2["device_ms"] / r2["iterations"],
                "product_ms": product_ms, "repeatable": r["lambda_min"] == r2["lambda_min"] and r["lambda_max"] == r2["lambda_max"]}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--which", type=int, nargs="+", default=[3, 0])
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    main(a.cells, a.which, a.reps)
