#!/usr/bin/env python
"""What the coupled multigrid preset buys: assemble + solve to rtol 1e-8 on hexahedra, k1 / k2 = 100, for growing beta, under
CG + pph_cmg (CG_CMG_PARAMS) next to the inexact Picard sweeps of the benchmark (PICARD_MG_INEXACT_SOLVER_PARAMS) and GMRES
under the multiplicative field split with multigrid-CG blocks (FIELDSPLIT_MG_PARAMS), on one build and one device.

Per configuration: one warm-up run, then `--repeats` runs of assembly + solve timed by the library's event pairs
(pph_get_timers: the assembly's own pair and the solve's); reported are the median and the spread (min .. max) of their sum,
the iterations or sweeps, and ms per cycle (CG + pph_cmg: the solve's ms over its iterations, one cycle each).  A preset that stops at its iteration /
sweep limit (`--cap`) is reported as such and not timed to the end.  Last, the fine-level coupled smoothing kernel alone
(pph_cmg_bench): ms per pass, its algorithmic bytes and the rate they amount to, and the set-up: on first use (with the
integration of K and M on every level) and after a re-assembly.

    python tools/cmg_probe.py --sizes 128 256 --out profiles/cmg_probe.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from perphil_amd import _ffi, solver_parameters as spar  # noqa: E402
from perphil_amd.solver import translate_options  # noqa: E402


def boundary_data(N):
    p = N + 1
    idx = np.arange(p ** 3, dtype=np.int64)
    i, j, k = idx % p, (idx // p) % p, idx // (p * p)
    b = np.nonzero((i == 0) | (i == N) | (j == 0) | (j == N) | (k == 0) | (k == N))[0]
    x, y, z = i[b] / N, j[b] / N, k[b] / N
    return b, np.exp(x) * np.sin(3 * y) + z, np.cos(2 * x) + y * y - 0.5 * z


def timed(ctx, cfg, coef, monolithic, repeats):
    """(median ms, min, max, median solve ms, iterations, inner iterations, converged) of assembly + solve over `repeats` runs after one warm-up."""
    ms, sol, info = [], [], None
    for rep in range(repeats + 1):
        ctx.assemble(*coef, monolithic=monolithic)
        _x, info, _h = ctx.solve(cfg, fetch=False, raise_on_diverged=False)
        t = ctx.timers()
        if rep > 0:
            ms.append(float(t["assemble_ms"] + t["solve_ms"]))
            sol.append(float(t["solve_ms"]))
        if not info.converged:
            break           # at its limit: reported, not repeated
    if not ms:
        ms, sol = [float("nan")], [float("nan")]
    return statistics.median(ms), min(ms), max(ms), statistics.median(sol), int(info.iterations), int(info.inner_iterations), bool(info.converged)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--betas", type=float, nargs="+", default=[1.0, 1e2, 1e4])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cap", type=int, default=200, help="iteration / sweep limit of the split presets")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("coupled multigrid probe: hexahedra, k1 = 1, k2 = 0.01, mu = 1, rtol 1e-8; ms = assembly + solve, median (min .. max) "
        f"of {args.repeats} runs after one warm-up")
    presets = [("CG + pph_cmg", spar.CG_CMG_PARAMS, False, True),
               ("Picard, inexact MG sweeps", {**spar.PICARD_MG_INEXACT_SOLVER_PARAMS, "snes_max_it": args.cap}, True, False),
               ("GMRES + field split, MG-CG blocks", {**spar.FIELDSPLIT_MG_PARAMS, "ksp_max_it": args.cap}, False, True)]
    for N in args.sizes:
        b, g1, g2 = boundary_data(N)
        with _ffi.Context(0) as ctx:
            ctx.mesh_build(3, _ffi.CELL_HEX, N, N, N)
            ctx.set_dirichlet(0, b, g1)
            ctx.set_dirichlet(1, b, g2)
            say(f"\nhex {N}^3: {2 * ctx.n} unknowns")
            # first use on this mesh: the hierarchy, K and M of every level integrated for the cycle, blocks and bounds
            ctx.assemble(1.0, 0.01, 1e2, 1.0, monolithic=True)
            first = ctx.cmg_bench(1)["setup_ms"]
            say(f"first set-up of the coupled cycle on the mesh (hierarchy + K and M of every level + blocks, one warm-up cycle): {first:.1f} ms")
            say(f"{'preset':36s} {'beta':>7s} {'its / sweeps':>13s} {'inner':>7s} {'ms':>30s} {'ms / cycle':>11s}")
            for beta in args.betas:
                coef = (1.0, 0.01, beta, 1.0)
                for label, opts, nonlinear, mono in presets:
                    cfg, _ = translate_options(opts, nonlinear=nonlinear)
                    med, lo, hi, solve_ms, its, inner, conv = timed(ctx, cfg, coef, mono, args.repeats)
                    if conv:
                        per = f"{solve_ms / its:.3f}" if label.startswith("CG + pph_cmg") and its else "-"
                        say(f"{label:36s} {beta:7g} {its:13d} {inner:7d} {f'{med:.2f} ({lo:.2f} .. {hi:.2f})':>30s} {per:>11s}")
                    else:
                        say(f"{label:36s} {beta:7g} {f'limit ({its})':>13s} {inner:7d} {'not converged: not timed':>30s} {'-':>11s}")
            ctx.assemble(1.0, 0.01, 1e2, 1.0, monolithic=True)
            r = ctx.cmg_bench(20)
            rate = r["step_bytes"] / (r["step_ms"] * 1e-3) / 1e12
            say(f"coupled smoothing kernel (fine level): {r['step_ms']:.3f} ms per pass, {r['step_bytes'] / 1e9:.3f} GB algorithmic "
                f"= {rate:.2f} TB/s; one cycle {r['cycle_ms']:.3f} ms; set-up after a re-assembly (K and M kept, one warm-up cycle) "
                f"{r['setup_ms']:.1f} ms")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
