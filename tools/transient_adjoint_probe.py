#!/usr/bin/env python3
"""Times of the transient adjoint at 128^3 Q1 hexahedra, CG_CMG_PARAMS, 20 steps, one mode per process (argument):
forward   the forward loop (pph_transient_steps_device);
backward  the backward loop (pph_transient_adjoint_device, dense G);
composed  the same sweep composed per step from pph_solve_rhs_device, pph_dpp_step_rhs_device and two pph_dpp_bilinear_device
          calls with torch arithmetic between them (it can yield only O0..O2);
kernel    pph_transient_bilinear_device alone (call time; kernel time comes from a kernel trace of this mode);
points    pph_eval_points_adjoint_device at 1000 and 4000 points: time per point from the difference.
Warm-up, then the median of the repetitions, host clock around work that ends in a device synchronise.  Prints one line
"TIMING {json}" (profiles/transient_adjoint_hex128.json collects them)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perphil_amd import _ffi, solver, solver_parameters as spar

mode = sys.argv[1]
NX, N = 128, 20
k1, k2, beta, mu, storage, theta, dt = 1.0, 0.01, 1.0, 1.0, (1.0, 1.0), 1.0, 0.01
ctx = _ffi.Context(0)
ctx.mesh_build(3, 2, NX, NX, NX)
n = ctx.n
P = NX + 1
idx = np.arange(n)
i, j, k = idx % P, (idx // P) % P, idx // (P * P)
bnd = idx[(i == 0) | (i == NX) | (j == 0) | (j == NX) | (k == 0) | (k == NX)]
for f in (0, 1):
    ctx.set_dirichlet(f, bnd, np.full(len(bnd), 1.0 - f))
cfg, _ = solver.translate_options(spar.CG_CMG_PARAMS)
ctx.transient_begin(k1, k2, beta, mu, storage, theta, dt)
gen = torch.Generator(device="cuda").manual_seed(3)
rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device="cuda", generator=gen)

def timed(fn, reps=3, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); out.append(time.perf_counter() - t)
    return statistics.median(out), out

p_init = rnd(2 * n)
res = {"mode": mode, "n": n}
if mode == "forward":
    def run():
        p = p_init.clone()
        d, infos, _ = ctx.transient_steps(cfg, p, N)
        res["iterations"] = [int(x.iterations) for x in infos]
    res["seconds"], res["all"] = timed(run)
elif mode in ("backward", "composed"):
    p = p_init.clone()
    _, _, _, traj = ctx.transient_steps(cfg, p, N, record=True)
    G = rnd(N + 1, 2 * n)
    if mode == "backward":
        def run():
            terms, q0, wsum, infos, done = ctx.transient_adjoint(cfg, traj, g=G)
            res["iterations"] = [int(x.iterations) for x in infos]
            res["terms0"] = terms[0].tolist()
        res["seconds"], res["all"] = timed(run)
    else:
        free = torch.ones(2 * n, dtype=torch.float64, device="cuda")
        tb = torch.from_numpy(bnd).cuda()
        free[tb] = 0.0; free[n + tb] = 0.0
        def run():
            q = free * G[N]
            wsum = torch.zeros_like(q)
            its = []
            for s in range(N - 1, -1, -1):
                w, info, _ = ctx.solve_rhs(cfg, q)
                its.append(int(info.iterations))
                b = ctx.step_rhs(w, k1, k2, beta, mu)
                d = traj[s + 1] - traj[s]
                o_p = ctx.dpp_bilinear(w, traj[s].contiguous())
                o_d = ctx.dpp_bilinear(w, d)
                terms = [a + theta * c for a, c in zip(o_p, o_d)]
                q = free * (G[s] + q + b)
                wsum += w
                if s == 0:
                    res["terms0"] = terms
            res["iterations"] = its
        res["seconds"], res["all"] = timed(run)
elif mode == "kernel":
    w, p0, p1 = rnd(2 * n), rnd(2 * n), rnd(2 * n)
    med, allt = timed(lambda: ctx.transient_bilinear(w, p0, p1, 0.5), reps=15, warm=3)
    nbox = NX ** 3
    nbytes = 32 * nbox + 48 * n
    res.update(seconds=med, all=allt, bytes=nbytes, gbytes_per_s=nbytes / med / 1e9)
    med2, _ = timed(lambda: ctx.dpp_bilinear(w, p0), reps=15, warm=3)
    res["dpp_bilinear_seconds"] = med2
elif mode == "points":
    out = {}
    for m in (1000, 4000):
        x = torch.rand(m, 3, dtype=torch.float64, device="cuda", generator=gen)
        c = rnd(m)
        out[m], _ = timed(lambda: ctx.eval_points_adjoint(x, c), reps=9, warm=2)
    res["seconds_by_m"] = out
    res["us_per_point"] = (out[4000] - out[1000]) / 3000 * 1e6
print("TIMING " + json.dumps(res), flush=True)
ctx.close()
