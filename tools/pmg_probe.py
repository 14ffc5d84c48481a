"""p-multigrid record for Q2 512^2 quads and Q2 64^3 hexes: hierarchy set-up time; one pc_apply(PC_PMG) with the tile kernels
of pph_pmg.hip ("pmg_fused" 1) and with the generic composition (0), split into the degree-2 level and the rest; bytes the
degree-2 passes move and their share of 8 TB/s; iterations and time of Picard + PMG and field-split GMRES + PMG to the
tolerance tools/p2_probe.py uses for GMRES + ILU(0) (1e-8), beside that ILU figure from the same run.
Writes <out>/pmg_<case>.json (default out: profiles/).  Usage: python tools/pmg_probe.py [case ...] [--out DIR] [--no-ilu]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from perphil_amd import _ffi, fd, solver_parameters as spar  # noqa: E402
from perphil_amd.solver import translate_options  # noqa: E402

CASES = {"q2_quad512": (2, _ffi.CELL_QUAD, 512, 512, 0), "q2_hex64": (3, _ffi.CELL_HEX, 64, 64, 64)}
PEAK = 8.0e12


def run(name, out_dir, with_ilu=True, reps=20):
    dim, kind, nx, ny, nz = CASES[name]
    out = {"case": name, "dim": dim, "kind": kind, "n": [nx, ny, nz], "mg_smooth": 2}
    with _ffi.Context(0) as ctx:
        ctx.mesh_build_lagrange(dim, kind, nx, ny, nz, 2)
        mesh = fd.Mesh(dim, kind, nx, ny, nz, comm=fd.COMM_SELF)
        b = mesh.boundary_nodes(degree=2)
        X = mesh.node_coordinates(b, degree=2)
        ctx.set_dirichlet(0, b, np.sin(np.pi * X[:, 0]) + X[:, 1])
        ctx.set_dirichlet(1, b, X[:, 0] * X[:, 1])
        ctx.assemble(1.0, 0.01, 1.0, 1.0, monolithic=True)
        out.update(nodes=ctx.n, nnz_block=ctx.nnzb)
        # nominal traffic of the four degree-2 passes of one cycle (two smoother steps, two residuals): matrix stream
        # 12 B per entry + 8 B per row pointer, and the vectors of the epilogues (56 / 56 / 25 / 24 B per row)
        nominal = 4 * (12.0 * ctx.nnzb + 8.0 * ctx.n) + (56.0 + 56.0 + 25.0 + 24.0) * ctx.n
        for fused in (1, 0):
            ctx.set_option("pmg_fused", fused)
            r = ctx.pc_bench(0, _ffi.PC_PMG, reps)
            key = "tile" if fused else "generic"
            if fused:
                out["hierarchy_setup_wall_ms"] = r["setup_ms"]      # (first call: includes the first cycle)
            out[f"apply_{key}_ms"] = r["apply_ms"]
            out[f"level0_{key}_ms"] = r["level0_ms"]
            out[f"rest_{key}_ms"] = r["apply_ms"] - r["level0_ms"]
            out[f"level0_{key}_frac_8TBs"] = nominal / (r["level0_ms"] * 1e-3) / PEAK
            if fused:
                out["level0_bytes_counted"] = r["level0_bytes"]
        out["level0_bytes_nominal"] = nominal
        if dim == 3:      # the variant of the tile kernels with 16 instead of 32 rows per tile (half the LDS per workgroup)
            ctx.set_option("pmg_fused", 1)
            ctx.set_option("pmg_tile_rows", 16)
            r = ctx.pc_bench(0, _ffi.PC_PMG, reps)
            out.update(apply_tile16_ms=r["apply_ms"], level0_tile16_ms=r["level0_ms"],
                       level0_tile16_frac_8TBs=nominal / (r["level0_ms"] * 1e-3) / PEAK)
            ctx.set_option("pmg_tile_rows", 32)
        ctx.set_option("pmg_fused", 1)
        for label, opts, nonlinear in [("picard_pmg", {**spar.PICARD_PMG_SOLVER_PARAMS, "snes_rtol": 1e-8}, True),
                                       ("fieldsplit_gmres_pmg", {**spar.FIELDSPLIT_PMG_PARAMS, "ksp_rtol": 1e-8}, False)]:
            cfg, _ = translate_options(opts, nonlinear=nonlinear)
            for rep in range(2):      # second run: hierarchy and work vectors in place
                x, info, _ = ctx.solve(cfg, fetch=False, raise_on_diverged=False)
                tm = ctx.timers()
            out[f"{label}_iterations"] = int(info.iterations)
            out[f"{label}_inner_iterations"] = int(info.inner_iterations)
            out[f"{label}_solve_ms"] = tm["solve_ms"]
            out[f"{label}_converged"] = bool(info.converged)
            out[f"{label}_resnorm"] = float(info.resnorm)
        if with_ilu:
            cfg, _ = translate_options({**spar.GMRES_ILU_PARAMS, "ksp_rtol": 1e-8, "ksp_max_it": 200})
            x, info, _ = ctx.solve(cfg, fetch=False, raise_on_diverged=False)
            tm = ctx.timers()
            out.update(gmres_ilu_iterations=int(info.iterations), gmres_ilu_solve_ms=tm["solve_ms"],
                       gmres_ilu_converged=bool(info.converged), gmres_ilu_resnorm=float(info.resnorm), gmres_ilu_max_it=200)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"pmg_{name}.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("cases", nargs="*", help=f"any of {', '.join(CASES)} (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of the JSON records")
    ap.add_argument("--no-ilu", action="store_true", help="leave the GMRES + ILU(0) comparison out (52 s at Q2 64^3)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    for c in args.cases:
        if c not in CASES:
            ap.error(f"unknown case {c!r}")
    for c in args.cases or list(CASES):
        run(c, args.out, with_ilu=not args.no_ilu, reps=args.reps)
