"""What the restated rate gradients G[s][k] = w_s^T F L_k lose when the backward solves run by the oracle's pcg (Jacobi, rtol
1e-13) instead of splu: the CPU figure behind SRC_GRAD_CPU_MEASURED in tests/test_transient_sources_gpu.py (the protocol of the
`terms` bar in tests/test_transient_adjoint_gpu.py).  Runs without a GPU over the degree-1 runs of that file and both theta:

  python tools/transient_sources_cpu_loss.py

Prints the loss of every run, of the absolute sums |w_s|^T |F L_k|, and the worst."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_transient_sources_gpu as G  # noqa: E402
import transient_adjoint_reference as A  # noqa: E402
import transient_sources_reference as S  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402


def main():
    worst = 0.0
    for run, (_, degree, name) in enumerate(G.STEP_RUNS):
        if degree != 1:
            continue      # (the degree-2 matrices are a device's export)
        for theta in (1.0, 0.5):
            pr = G._step_problem(run, theta)
            Gf = np.random.default_rng(90 + run).standard_normal((G.N_STEPS + 1, 2 * pr["n"]))
            args = (pr["K"], pr["M"], G.CF, G.STORAGE, theta, G.DT, pr["masks"], list(pr["states"]), Gf)
            Top = A.step_operator(pr["K"], pr["M"], G.CF, G.STORAGE, theta, G.DT, pr["masks"]).tocsr()
            pcg = lambda b: o.pcg(Top, b, o.jacobi_apply(Top), rtol=1e-13, atol=1e-300, max_it=100000).x
            G1, Gs = S.source_gradients(A.adjoint_sweep(*args), pr["loads"], pr["masks"])
            G2, _ = S.source_gradients(A.adjoint_sweep(*args, solve=pcg), pr["loads"], pr["masks"])
            e = float((np.abs(G1 - G2) / np.maximum(Gs, 1e-300)).max())
            worst = max(worst, e)
            print(f"{G._rid(run)} theta {theta}: {e:.2e}")
    print(f"worst {worst:.2e}")


if __name__ == "__main__":
    main()
