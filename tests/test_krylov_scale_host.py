"""Host checks of tests/krylov_reference.py, the reference behind tests/test_krylov_scale_gpu.py: the restated loops against
SciPy and the oracle on the small meshes of asm_scale_reference, the preconditioner vectors against the CSR of the same blocks, the
restated launch rules at their thresholds, and - on every large case of the GPU file - stand-ins for wrong kernels (one vector
operation at a time leaves out the rows of its last grid-stride pass) that the GPU file's comparison must reject by a factor of
at least 1000.

Tolerances of the small-mesh comparisons.
  solution     both loops run to rtol 1e-12 in the preconditioned norm; |x - spsolve| / max |x| <= 1e-12 kappa(P^-1 A) is what
               that residual allows; the small systems here have kappa below 1e3: SOLVE = 1e-9.
  CG history   the oracle's pcg is the same recurrence with the matrix in CSR: the two differ by the rounding of the products
               and sums (a few eps per operation), which CG carries forward amplified by at most kappa per iteration in the
               worst case and by far less in practice; compared over the first 8 iterations (as long as the
               history stays above 1e-8 of its first entry): HISTORY = 1e-10.
  vectors      1 / diag: two roundings apart from 1 / (the CSR diagonal), whose entries are themselves a few eps from the
               gather's: 16 eps.  The 2 x 2 inverses: 32 eps cond(block) per node, against numpy.linalg.inv.
Measured: the printouts, and tests/README_krylov_scale.md."""
import os
import sys
import time

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import asm_scale_reference as R  # noqa: E402
import krylov_reference as K  # noqa: E402
import transient_reference as T  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

EPS = K.EPS
SOLVE, HISTORY = 1e-9, 1e-10
MUTANT_FACTOR = 1000.0


def _id(c):
    return R.NAMES[c[0]] + "x".join(str(q) for q in c[1])


def _csr(c):
    nd = c["nd"]
    Km, Mm = T.matfree_scalar_matrices(c["kind"], nd[0], nd[1], nd[2] if len(nd) == 3 else 0)
    return T.shifted_blocks(Km, Mm, R.CF, (0.0, 0.0), c["masks"], c["g"])[:4]


@pytest.mark.parametrize("case", R.SMALL, ids=_id)
def test_restated_loops_against_scipy_and_the_oracle(case):
    c = K.setup(*case)
    A11, A22, A12, A21 = _csr(c)
    A = sp.bmat([[A11, A12], [A21, A22]], format="csr")
    xs = spla.spsolve(A.tocsc(), c["b"])
    S = K.system(c)
    worst = [0.0, 0.0]
    for pc in ("none", "jacobi", "block2"):
        # (restarts: GMRES(3) without a preconditioner stagnates on these systems - the short cycle is run preconditioned)
        for ksp, restart in (("cg", 0), ("gmres", 30)) + ((("gmres", 3),) if pc != "none" else ()):
            out = K.run(c, ksp, pc, restart, 2000, 1e-12, 0.0)
            assert out.converged and not out.breakdown, (ksp, pc, restart)
            err = float(abs(out.x - xs).max() / abs(xs).max())
            worst[0] = max(worst[0], err)
            assert err <= SOLVE, (ksp, pc, restart, err)
            assert not out.x[~c["free"]].any()
        # the oracle's pcg with the same preconditioner as a function
        P = K.preconditioner(S, pc)
        M_apply = None if P is None else (P if callable(P) else (lambda v, P=P: P * v))
        ref = o.pcg(A, c["b"], M_apply, rtol=1e-12, atol=0.0, max_it=2000)
        mine = K.run(c, "cg", pc, 0, 2000, 1e-12, 0.0)
        # (entries of a Krylov space that is not yet exhausted: on two free rows the third entry is rounding over rounding)
        m = min(9, len(ref.history), len(mine.hist), int(np.argmax(np.array(ref.history + [0.0]) <= 1e-8 * ref.history[0])))
        assert m >= min(3, int(c["free"].sum()))     # (with `free` rows: entries 0 .. free - 1)
        d = K.hist_distance(mine.hist[:m], np.array(ref.history[:m]))
        worst[1] = max(worst[1], d)
        assert d <= HISTORY, (pc, d)
        assert abs(mine.iterations - ref.its) <= 1
    print(f"{_id(case)}: |x - spsolve| / max |x| {worst[0]:.1e} (bar {SOLVE:g}); CG history against the oracle's pcg {worst[1]:.1e} (bar {HISTORY:g})")


@pytest.mark.parametrize("case", R.SMALL, ids=_id)
def test_preconditioner_vectors_against_the_csr(case):
    c = K.setup(*case)
    A11, A22, A12, A21 = _csr(c)
    S = K.system(c)
    dj = K.jacobi_vector(S)
    want = 1.0 / np.concatenate([A11.diagonal(), A22.diagonal()])
    ej = float((abs(dj - want) / abs(want)).max())
    assert ej <= 16 * EPS and np.all(dj[~c["free"]] == 1.0)
    b = K.block2_vectors(S)
    worst = 0.0
    d = [A11.diagonal(), A12.diagonal(), A21.diagonal(), A22.diagonal()]
    for i in range(c["n"]):
        blk = np.array([[d[0][i], d[1][i]], [d[2][i], d[3][i]]])
        inv = np.linalg.inv(blk)
        got = np.array([[b[0][i], b[1][i]], [b[2][i], b[3][i]]])
        frac = float(abs(got - inv).max() / abs(inv).max() / (32 * EPS * np.linalg.cond(blk)))
        worst = max(worst, frac)
    assert worst <= 1.0
    # the application is the product with those blocks
    r = np.random.default_rng(3).standard_normal(2 * c["n"])
    z = K.block2_apply(b)(r)
    n = c["n"]
    assert np.array_equal(z[:n], b[0] * r[:n] + b[1] * r[n:]) and np.array_equal(z[n:], b[2] * r[:n] + b[3] * r[n:])
    print(f"{_id(case)}: 1 / diag {ej / EPS:.1f} eps from the CSR's (bar 16); 2 x 2 inverses at {worst:.3f} of 32 eps cond")


def test_perturbed_system_is_a_few_eps_away():
    c = K.setup(R.QUAD, (5, 3))
    S = K.system(c)
    x = np.random.default_rng(2).standard_normal(2 * c["n"])
    y, yp = S.apply("MONO", x), K.perturbed(S, 9).apply("MONO", x)
    rel = abs(yp - y) / np.where(y != 0, abs(y), 1.0)
    assert 0 < rel.max() <= 5 * EPS and np.median(rel) > 0.5 * EPS       # (4 eps |xi| and the rounding of the product)
    a, b = K.perturbed(S, 9), K.perturbed(S, 9)
    assert np.array_equal(a.apply("MONO", x), b.apply("MONO", x))


@pytest.mark.parametrize("case", R.SMALL + [(R.QUAD, (1024, 512)), (R.HEX, (128, 64, 64))], ids=_id)
def test_longdouble_box_matrices(case):
    """box_matrices_longdouble is transient_reference.box_matrices evaluated in longdouble: the fp64 ones are its rounding to
    within 2 eps of the largest entry (a third or a sixth rounded once, then two to four products and a sum), they are not
    identical (or the longdouble run would hold nothing of the operator's fp64 form), and the longdouble ones keep the
    exact properties - symmetric, stiffness rows summing to 0, mass summing to the box volume - to 64 longdouble eps."""
    kind, nd = case
    KB, MB = T.box_matrices(kind, list(nd))
    KL, ML = K.box_matrices_longdouble(kind, list(nd))
    assert KL.dtype == np.longdouble and ML.dtype == np.longdouble
    dk, dm = float(abs(KB - KL).max() / abs(KL).max()), float(abs(MB - ML).max() / abs(ML).max())
    assert dk <= 2 * EPS and dm <= 2 * EPS and (dk > 0 or dm > 0), (dk, dm)
    tiny = 64 * float(np.finfo(np.longdouble).eps)
    assert np.array_equal(KL, KL.T) and np.array_equal(ML, ML.T)
    assert float(abs(KL.sum(axis=1)).max() / abs(KL).max()) <= tiny
    assert float(abs(ML.sum() * np.longdouble(int(np.prod(nd))) - 1)) <= tiny
    print(f"{_id(case)}: fp64 box matrices {dk / EPS:.2f} eps (K), {dm / EPS:.2f} eps (M) of the largest entry from the longdouble ones")


def test_launch_rules_at_their_thresholds():
    # ew_grid: two entries per thread up to 2048 workgroups; a third pass begins at N > 1 048 576
    assert K.la_launch(1)["grid"] == 1 and K.la_launch(512)["grid"] == 1 and K.la_launch(513)["grid"] == 2
    assert K.la_launch(1048576) == {"grid": 2048, "passes": 2, "last": 524288, "red_grid": 1024, "red_passes": 4, "red_last": 262144, "partials": 1024}
    L = K.la_launch(1048577)
    assert (L["passes"], L["last"], L["red_passes"], L["red_last"]) == (3, 1, 5, 1)
    assert K.la_launch(524288)["red_grid"] == 1024 and K.la_launch(524287)["red_grid"] == 1024 and K.la_launch(523776)["red_grid"] == 1023
    # k_block2_build: one node per thread, 2048 workgroups
    assert K.block2_launch(524288)["build_passes"] == 1 and K.block2_launch(524289)["build_passes"] == 2
    assert K.block2_launch(1048576)["passes"] == 2 and K.block2_launch(1048577)["passes"] == 3
    assert [K.mdot_widths(k) for k in range(1, 8)] == [(1,), (2,), (2, 1), (4,), (4, 1), (4, 2), (4, 2, 1)]
    assert K.mdot_widths(31) == (4,) * 7 + (2, 1)
    Sp = K.spmv_launch(1090050, 54)
    assert (Sp["lanes"], Sp["grid"], Sp["chunks"], Sp["steps"]) == (8, 1024, 34065, 2)
    assert K.spmv_launch(1000, 13)["lanes"] == 4 and K.spmv_launch(1000, 14)["lanes"] == 8 and K.spmv_launch(1000, 18, lanes=16)["lanes"] == 16
    assert K.spmv_launch(1051650, 18, blocks=2048)["grid"] == 2048 and K.spmv_launch(100, 18)["grid"] == 8


def test_two_fp64_assemblies_of_one_system_in_the_loops():
    """Why the longdouble run behind the GPU file's bar holds its box matrices in longdouble.  The matrix-free restatement never
    forms an assembled entry; an assembled matrix stores every entry as an fp64-rounded sum over its cells.  Both are correct to
    half an ulp per entry, and the products differ by a few eps of (|A| |x|)_i - but that difference is the same in every product
    of a loop, and relative to |A| |x|, not to A x.  `perturbed` (seeded anew per product, relative to A x) does not model it, and
    a longdouble run on the fp64 box matrices has the fp64 run's operator.  Here, without a device: the restated loops on the fp64
    CSR of transient_reference (the entry-wise reference of tests/test_asm_scale_gpu.py) against the matrix-free restatement,
    quad 1024x512.  An independent correct fp64 assembly must be within the bars of the matrix-free comparison (asserted; measured
    0.03 of a bar), and for Jacobi-CG it is NOT within bars_loop, the bar of the loop's rounding alone (asserted: 1.78e-13
    against 1.0e-13) - which is why the GPU file uses bars_loop only where both sides hold one stored matrix."""
    kind, nd = K.LARGE["quad1024x512"]
    c = K.setup(kind, nd)
    A11, A22, A12, A21 = _csr(c)
    A = sp.bmat([[A11, A12], [A21, A22]], format="csr")
    S = K.system(c)
    v = np.random.default_rng(1).standard_normal(A.shape[0]) * c["free"]
    mag = S.apply("MONO", v, True)
    prod = float((abs(A @ v - S.apply("MONO", v)) / np.where(mag > 0, mag, 1.0)).max() / EPS)
    assert prod <= 32        # RESTATED of tests/test_asm_scale_host.py
    for loop in (("cg", "jacobi", 0, 6), ("cg", "none", 0, 6), ("gmres", "jacobi", 7, 10)):
        ref = K.reference(c, *loop)
        out = K.run_on_matrix(A, c["b"], *loop)
        dh, dx = K.hist_distance(out.hist, ref["hist"]), K.x_distance(out.x, ref["x"])
        print(f"quad1024x512 {loop[0]} {loop[1]}: the loop on an assembled fp64 CSR against the matrix-free restatement: history {dh:.2e} = "
              f"{dh / ref['bars'][0]:.2f} bars, iterate {dx:.2e} = {dx / ref['bars'][1]:.2f} bars (products differ by {prod:.1f} eps |A||x|)")
        assert out.iterations == ref["out"].iterations and dh <= ref["bars"][0] and dx <= ref["bars"][1]
        if loop == ("cg", "jacobi", 0, 6):
            assert dh > ref["bars_loop"][0] and dx > ref["bars_loop"][1], (dh, dx, ref["bars_loop"])


# -- mutants: one vector kernel loses the rows of its last pass ---------------------------------------------------------------
class Mutant(K.Ops):
    """`op` leaves out the rows of `tail` (a mask over the 2n entries): a reduction does not add them, an update does not
    write them."""

    def __init__(self, op, tail):
        self.op, self.keep = op, ~tail

    def spmv_dot(self, p, q):
        return np.dot(p[self.keep], q[self.keep]) if self.op == "spmv_dot" else np.dot(p, q)

    def mdot(self, V, w):
        h = [np.dot(v, w) for v in V]
        if self.op == "mdot":      # one dot product of the multi-dot: the first
            h[0] = np.dot(V[0][self.keep], w[self.keep])
        return h

    def dot2(self, r, z):
        if self.op != "dot2":
            return K.Ops.dot2(self, r, z)
        return np.dot(r[self.keep], z[self.keep]), np.dot(z[self.keep], z[self.keep])

    def maxpy(self, w, V, h, sign):
        if self.op != "maxpy":
            return K.Ops.maxpy(self, w, V, h, sign)
        old = w.copy()
        K.Ops.maxpy(self, w, V, h, sign)
        w[~self.keep] = old[~self.keep]

    def cg_update(self, x, r, p, q, alpha, dinv):
        if self.op != "cg_update":
            return K.Ops.cg_update(self, x, r, p, q, alpha, dinv)
        k = self.keep
        x[k] += alpha * p[k]
        r[k] -= alpha * q[k]
        z = dinv * r if dinv is not None else r.copy()     # (on the rows left out: dinv .* the old r, the old z)
        return z, np.dot(r[k], z[k]), np.dot(z[k], z[k])

    def axpby(self, p, z, beta):
        if self.op != "axpby":
            return K.Ops.axpby(self, p, z, beta)
        old = p.copy()
        K.Ops.axpby(self, p, z, beta)
        p[~self.keep] = old[~self.keep]


# (mesh): [(operation, loop it is left out of)]
_CGJ, _CGB, _GMJ = ("cg", "jacobi", 0, 6), ("cg", "block2", 0, 6), ("gmres", "jacobi", 7, 10)
MUTANTS = {
    "quad1024x512": [("mdot", _GMJ), ("maxpy", _GMJ), ("dot2", _CGB), ("cg_update", _CGJ), ("block2", _CGB), ("axpby", _CGJ)],
    "quad2048x512": [("mdot", ("gmres", "block2", 3, 4)), ("maxpy", ("gmres", "block2", 3, 4)), ("block2", ("gmres", "block2", 3, 4)),
                     ("dot2", ("cg", "block2", 0, 3)), ("block2", ("cg", "block2", 0, 3)), ("axpby", ("cg", "block2", 0, 3))],
    "hex128x64x64": [("cg_update", ("cg", "jacobi", 0, 3)), ("axpby", ("cg", "jacobi", 0, 3)), ("spmv_dot", ("cg", "jacobi", 0, 3))],
}
FREE_IN_TAIL = {"quad1024x512": (2047, 3074)}


@pytest.mark.parametrize("mesh", list(K.LARGE))
def test_mutants_miss_the_bars_of_the_large_cases(mesh):
    """Every loop a mutant is tried on appears among the GPU file's loops of that mesh; its bar is the GPU file's
    (krylov_reference.reference).  The block-2 mutant leaves out the nodes of the last pass of the block-2 kernel that is past its
    cap on that mesh: k_block2_build on quad 1024x512 (1 537 nodes), k_block2 on quad 2048x512 (2 561 nodes)."""
    t0 = time.time()
    kind, nd = K.LARGE[mesh]
    c = K.setup(kind, nd)
    n, N = c["n"], 2 * c["n"]
    L, B = K.la_launch(N), K.block2_launch(n)
    assert L["passes"] >= 3 and L["last"] == L["red_last"] and L["red_grid"] == K.RED_BLOCKS
    tail = K.tail_mask(N, L["last"])
    live = int(np.count_nonzero(c["b"][tail]))
    assert live > 0                                  # the last pass holds free rows on which b is nonzero
    if mesh in FREE_IN_TAIL:
        assert (live, L["last"]) == FREE_IN_TAIL[mesh]
    nodes, live_nodes = np.zeros(n, dtype=bool), 0
    if any(op == "block2" for op, _ in MUTANTS[mesh]):
        nodes = K.tail_mask(n, B["last"] if B["passes"] >= 3 else B["build_last"])
        assert (B["passes"] >= 3 or B["build_passes"] >= 2) and 0 < nodes.sum() < 4096
        live_nodes = int(np.count_nonzero(c["b"][:n][nodes] != 0) + np.count_nonzero(c["b"][n:][nodes] != 0))
        assert live_nodes > 0
    lines = []
    for op, loop in MUTANTS[mesh]:
        assert loop in K.LOOPS[mesh]
        ref = K.reference(c, *loop)
        bar_h, bar_x = ref["bars"]
        if op == "block2":
            mut = K.run(c, *loop, skip=nodes)
        else:
            mut = K.run(c, *loop, ops=Mutant(op, tail))
        fh, fx = K.hist_distance(mut.hist, ref["hist"]) / bar_h, K.x_distance(mut.x, ref["x"]) / bar_x
        lines.append(f"  {op:10s} left out of {loop[0]} {loop[1]}: history {fh:.2e} bars, iterate {fx:.2e} bars (bars {bar_h:.1e} / {bar_x:.1e})")
        print(lines[-1], flush=True)
        assert max(fh, fx) >= MUTANT_FACTOR, (mesh, op, loop, fh, fx)
    print(f"{mesh}: last pass {L['last']} rows of {N} ({live} free with b != 0); block-2 nodes left out {int(nodes.sum())} ({live_nodes} free entries with b != 0); {time.time() - t0:.1f} s")
