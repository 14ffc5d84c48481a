"""Degree-2 record: assembly time (pattern, K/M, blocks), pph_spmv_bench of A11 and the monolithic matrix with the fraction
of 8 TB/s over the bytes really streamed (12 B per entry + row pointers + x, y), and GMRES + ILU(0) iterations and time,
for Q2 512^2 quads and Q2 64^3 hexes.  Writes <out>/p2_<case>.json (default out: profiles/).  Usage: python tools/p2_probe.py [case ...] [--out DIR]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from perphil_amd import _ffi, fd, solver_parameters as spar  # noqa: E402
from perphil_amd.solver import translate_options  # noqa: E402

CASES = {"q2_quad512": (2, _ffi.CELL_QUAD, 512, 512, 0), "q2_hex64": (3, _ffi.CELL_HEX, 64, 64, 64)}
PEAK = 8.0e12


def run(name, out_dir):
    dim, kind, nx, ny, nz = CASES[name]
    out = {"case": name, "dim": dim, "kind": kind, "n": [nx, ny, nz]}
    with _ffi.Context(0) as ctx:
        t0 = time.perf_counter()
        ctx.mesh_build_lagrange(dim, kind, nx, ny, nz, 2)
        out["mesh_pattern_wall_ms"] = (time.perf_counter() - t0) * 1e3
        mesh = fd.Mesh(dim, kind, nx, ny, nz, comm=fd.COMM_SELF)
        b = mesh.boundary_nodes(degree=2)
        X = mesh.node_coordinates(b, degree=2)
        ctx.set_dirichlet(0, b, np.sin(np.pi * X[:, 0]) + X[:, 1])
        ctx.set_dirichlet(1, b, X[:, 0] * X[:, 1])
        ctx.assemble(1.0, 0.01, 1.0, 1.0, monolithic=True)
        tm = ctx.timers()
        out.update(nodes=ctx.n, nnz_block=ctx.nnzb, mesh_ms=tm["mesh_ms"], km_ms=tm["assemble_ms"], blocks_ms=tm["bc_blocks_ms"])
        out["km_bytes_written"] = 16.0 * ctx.nnzb
        for which, label, rows, nnz in [(_ffi.MAT_A11, "A11", ctx.n, ctx.nnzb), (_ffi.MAT_MONO, "mono", 2 * ctx.n, 4 * ctx.nnzb)]:
            ms = ctx.spmv_bench(which, 50)
            byts = 12.0 * nnz + 8.0 * (rows + 1) + 16.0 * rows
            out[f"spmv_{label}_ms"] = ms
            out[f"spmv_{label}_bytes"] = byts
            out[f"spmv_{label}_frac_8TBs"] = byts / (ms * 1e-3) / PEAK
        # GMRES(30) + ILU(0), capped at 200 iterations: the record is the time per iteration and the residual reached
        cfg, _ = translate_options({**spar.GMRES_ILU_PARAMS, "ksp_rtol": 1e-8, "ksp_max_it": 200})
        x, info, _ = ctx.solve(cfg, raise_on_diverged=False)
        tm = ctx.timers()
        out.update(gmres_ilu_iterations=int(info.iterations), gmres_ilu_solve_ms=tm["solve_ms"], converged=bool(info.converged),
                   gmres_ilu_resnorm=float(info.resnorm), gmres_ilu_max_it=200)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"p2_{name}.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("cases", nargs="*", help=f"any of {', '.join(CASES)} (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of the JSON records")
    args = ap.parse_args()
    for c in args.cases:
        if c not in CASES:
            ap.error(f"unknown case {c!r}")
    for c in args.cases or list(CASES):
        run(c, args.out)
