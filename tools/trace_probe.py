#!/usr/bin/env python
"""What pathline tracing costs: the projected Darcy velocity of the manufactured macro pressure on hexahedra, seeds uniform
in the cube, RK4 with a step chosen so that the median path takes about `--median-steps` steps, everything on the device
(postprocessing.trace_pathlines with a device-resident velocity and device seeds).

Per mesh: one pilot run on a tenth of the seeds fixes dt; then, for every chunk of `--chunks` and for chunk = max_steps
(one launch, no compaction: what the default chunk of 4096 amounts to here): one warm-up call and `--repeats` timed calls
(host clock around the call, which returns after the stream has finished) - median ms per call (min .. max),
particle-steps per second, and the launches (ceil(longest path / chunk)).  Every chunk must give the same bits; the probe
checks that.

    python tools/trace_probe.py --sizes 64 128 --out profiles/trace_probe.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from perphil_amd import DPPParameters, fd, postprocessing as pp  # noqa: E402
from perphil_amd.manufactured_solutions import exact_expressions_3d  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--seeds", type=int, default=1000000)
    ap.add_argument("--median-steps", type=int, default=300)
    ap.add_argument("--max-steps", type=int, default=4000)
    ap.add_argument("--chunks", type=int, nargs="*", default=[16, 64, 256, 1024, 2048])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    params = DPPParameters()
    say(f"pathline probe: hexahedra, velocity of the manufactured macro pressure (k1 / mu = {float(params.k1) / float(params.mu):g}), "
        f"{args.seeds} seeds uniform in the cube, max_steps {args.max_steps}; ms per call = median (min .. max) of {args.repeats} "
        "calls after one warm-up")
    for N in args.sizes:
        mesh = fd.UnitCubeMesh(N, N, N, hexahedral=True, comm=fd.COMM_SELF)
        V = fd.FunctionSpace(mesh, "CG", 1)
        _u1, p1, _u2, _p2 = exact_expressions_3d(mesh, params)
        dev = mesh.context().torch_device()
        p = fd.Function(V, torch.from_numpy(p1(mesh.local_node_coordinates())).to(dev))
        u = pp.calculate_darcy_velocity_from_pressure(p, float(params.k1) / float(params.mu))
        seeds = torch.from_numpy(np.random.default_rng(1).random((args.seeds, 3))).to(dev)
        speed = float(u.torch().reshape(-1, 3).norm(dim=1).median())
        dt = 0.5 / (args.median_steps * speed)
        pilot = pp.trace_pathlines(u, seeds[: max(1, args.seeds // 10)].contiguous(), dt, args.max_steps)
        dt *= float(pilot.steps.double().median()) / args.median_steps
        say(f"\nhex {N}^3: {mesh.num_vertices()} nodes, median nodal speed {speed:.3g}, dt {dt:.3g}")
        say(f"{'chunk':>10s} {'launches':>9s} {'ms per call':>28s} {'particle-steps / s':>20s}")
        base = None
        for chunk in [c for c in args.chunks if c < args.max_steps] + [args.max_steps]:
            ms, r = [], None
            for rep in range(args.repeats + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = pp.trace_pathlines(u, seeds, dt, args.max_steps, chunk=chunk)
                torch.cuda.synchronize()
                if rep:
                    ms.append((time.perf_counter() - t0) * 1e3)
            steps = int(r.steps.sum())
            launches = -(-int(r.steps.max()) // chunk)
            med = statistics.median(ms)
            label = f"{chunk}" + (" (none)" if chunk == args.max_steps else "")
            say(f"{label:>10s} {launches:9d} {f'{med:.2f} ({min(ms):.2f} .. {max(ms):.2f})':>28s} {steps / (med * 1e-3):20.4g}")
            if base is None:
                base = r
                say(f"{'':>10s} median steps {int(r.steps.double().median())}, longest {int(r.steps.max())}, total {steps}; "
                    f"counts {r.counts}")
            else:
                same = all(torch.equal(a, b) for a, b in ((r.steps, base.steps), (r.status, base.status), (r.side, base.side)))
                same = same and all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
                                    for a, b in ((r.end, base.end), (r.time, base.time), (r.length, base.length)))
                if not same:
                    raise SystemExit(f"chunk {chunk} changed the results")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
