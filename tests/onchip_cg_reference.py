"""NumPy restatement of the on-chip LU-equivalent block solve (`k_coarse_cg_sell` through `mg_onchip_cg`, pph_mg.hip) and of
the direct-equivalent solve built on it, for `test_onchip_block_solve_host.py` and `test_onchip_block_solve_gpu.py`.

The kernel: Jacobi-preconditioned CG from a zero guess on one scalar block, test ||D^-1 r||_2 <= rtol ||D^-1 b||_2 on the
recurrence residual, stop on p.Ap <= 0, at most 8 n + 64 iterations (option "onchip_max_it"), a zero right-hand side is
converged at once.  Placed inside the oracle's GMRES as the block solves of the multiplicative field split, the whole solve that
`translate_options` configures for LINEAR_SOLVER_PARAMS / FIELDSPLIT_LU_PARAMS is a CPU computation."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import dpp_oracle as o

ONCHIP_MAX_ROWS = 4096          # BlockSolver::solve: blocks of at most this many rows are solved on chip
ONCHIP_RTOL = 1e-12             # min(cfg.inner_rtol, 1e-12) with the inner_rtol 1e-12 both presets translate to

# (label, dim, kind, nx, ny, nz): the branch each mesh is there for is named in tests/README.md
MESHES = [
    ("quad 63x63", 2, o.CELL_QUAD, 63, 63, 0),
    ("quad 64x64", 2, o.CELL_QUAD, 64, 64, 0),
    ("quad 127x31", 2, o.CELL_QUAD, 127, 31, 0),
    ("quad 15x15", 2, o.CELL_QUAD, 15, 15, 0),
    ("quad 16x15", 2, o.CELL_QUAD, 16, 15, 0),
    ("quad 1x1", 2, o.CELL_QUAD, 1, 1, 0),
    ("quad 2x2", 2, o.CELL_QUAD, 2, 2, 0),
    ("tri 63x63", 2, o.CELL_TRI, 63, 63, 0),
    ("tri 20x11", 2, o.CELL_TRI, 20, 11, 0),
    ("hex 15x15x15", 3, o.CELL_HEX, 15, 15, 15),
    ("hex 31x7x15", 3, o.CELL_HEX, 31, 7, 15),
    ("hex 5x4x6", 3, o.CELL_HEX, 5, 4, 6),
    ("hex 1x1x1", 3, o.CELL_HEX, 1, 1, 1),
    ("tet 15x15x15", 3, o.CELL_TET, 15, 15, 15),
    ("tet 7x9x5", 3, o.CELL_TET, 7, 9, 5),
]
NODES = {"quad 63x63": 4096, "quad 64x64": 4225, "quad 127x31": 4096, "quad 15x15": 256, "quad 16x15": 272, "quad 1x1": 4,
         "quad 2x2": 9, "tri 63x63": 4096, "tri 20x11": 252, "hex 15x15x15": 4096, "hex 31x7x15": 4096, "hex 5x4x6": 210,
         "hex 1x1x1": 8, "tet 15x15x15": 4096, "tet 7x9x5": 480}
THRESHOLD_MESHES = ("quad 63x63", "tri 63x63", "hex 15x15x15", "tet 15x15x15")
BASE_COEFFS = (1.0, 1e-2, 1.0, 1.0)                                # (k1, k2, beta, mu)
EXTRA_COEFFS = ((1.0, 1e-4, 1.0, 1.0), (1.0, 1e-2, 100.0, 1.0))    # on the threshold meshes only
CASES = [(m[0], BASE_COEFFS) for m in MESHES] + [(lbl, c) for lbl in THRESHOLD_MESHES for c in EXTRA_COEFFS]
_BY_LABEL = {m[0]: m for m in MESHES}

# outer Krylov settings that perphil_amd.solver.translate_options produces: LINEAR_SOLVER_PARAMS ("direct") and
# {**GMRES_PARAMS, **FIELDSPLIT_LU_PARAMS} ("fieldsplit_lu"); test_onchip_block_solve_host.py checks them against it
PRESETS = {"direct": dict(rtol=1e-13, atol=1e-300, max_it=200, restart=30),
           "fieldsplit_lu": dict(rtol=1e-8, atol=1e-12, max_it=50000, restart=30)}


def case_id(label, coeffs):
    return f"{label.replace(' ', '-')}-k2={coeffs[1]:g}-beta={coeffs[2]:g}"


def params_of(coeffs):
    return o.Params(k1=coeffs[0], k2=coeffs[1], beta=coeffs[2], mu=coeffs[3])


@lru_cache(maxsize=None)
def system(label, coeffs):
    """(oracle mesh, oracle system with the manufactured solution on the whole boundary) - computed once, not modified."""
    _, dim, kind, nx, ny, nz = _BY_LABEL[label]
    om = o.build_mesh(dim, kind, nx, ny, nz)
    assert om.num_nodes == NODES[label]
    return om, o.build_system(om, params_of(coeffs), mms=True)


def jacobi_cg(A, b, rtol=ONCHIP_RTOL, max_it=None):
    """The kernel's loop.  Returns (x, iterations = updates of x, converged)."""
    n = A.shape[0]
    if max_it is None:
        max_it = 8 * n + 64
    dinv = 1.0 / A.diagonal()
    x = np.zeros(n)
    r = b.astype(np.float64).copy()
    z = dinv * r
    p = z.copy()
    zz, rz = float(z @ z), float(r @ z)
    tol = rtol * np.sqrt(zz)
    if not np.sqrt(zz) > tol:
        return x, 0, zz == 0.0
    for it in range(max_it):
        q = A @ p
        pq = float(p @ q)
        if not pq > 0.0:
            return x, it, False
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        z = dinv * r
        zz2, rz2 = float(z @ z), float(r @ z)
        if np.sqrt(zz2) <= tol:
            return x, it + 1, True
        p = z + (rz2 / rz) * p
        rz = rz2
    return x, max_it, False


@dataclass
class BlockStats:
    solves: int = 0
    unconverged: int = 0
    cg_iterations: int = 0
    per_solve: list = field(default_factory=list)


def fieldsplit_onchip_apply(A, n, stats, rtol=ONCHIP_RTOL, max_it=None):
    """Multiplicative field split (z1 = A11^-1 r1 ; z2 = A22^-1 (r2 - A21 z1)) with the restated on-chip block solves."""
    A = A.tocsr()
    A11, A22, A21 = A[:n, :n].tocsr(), A[n:, n:].tocsr(), A[n:, :n].tocsr()

    def block(Ab, rhs):
        x, its, ok = jacobi_cg(Ab, rhs, rtol, max_it)
        stats.solves += 1
        stats.unconverged += 0 if ok else 1
        stats.cg_iterations += its
        stats.per_solve.append(its)
        return x

    def apply(v):
        z1 = block(A11, v[:n])
        z2 = block(A22, v[n:] - A21 @ z1)
        return np.concatenate([z1, z2])

    return apply


@dataclass
class Restated:
    x: np.ndarray              # u0 + du
    outer_its: int
    history: list
    converged: bool
    stats: BlockStats
    outer_its_allowed: tuple   # counts a device run may report (see outer_counts_allowed)


def outer_counts_allowed(history, tol, its, noise):
    """Outer iteration counts that an equally valid evaluation of the same algorithm can report.  The block solves are
    accurate to ONCHIP_RTOL only, so two evaluations that differ in rounding (the workgroup's reduction order against
    NumPy's) produce preconditioned residual norms that differ by up to `noise` = rtol_inner * history[0] in absolute terms.
    The count is the first k with history[k] <= tol: it is certain where history[k] + noise <= tol and history[k-1] - noise >
    tol; otherwise the crossing can happen one iteration earlier or later."""
    allowed = {its}
    if its >= 1 and history[its - 1] - noise <= tol:
        allowed.add(its - 1)
    if history[its] + noise > tol:
        allowed.add(its + 1)
    return tuple(sorted(allowed))


@lru_cache(maxsize=None)
def restated_solve(label, coeffs, preset, onchip_max_it=None):
    """The direct-equivalent solve as the device runs it, in NumPy."""
    _, osys = system(label, coeffs)
    kw = PRESETS[preset]
    stats = BlockStats()
    apply = fieldsplit_onchip_apply(osys.A, osys.n, stats, max_it=onchip_max_it)
    res = o.gmres(osys.A, osys.rhs, apply, **kw)
    tol = max(kw["rtol"] * res.history[0], kw["atol"])
    allowed = outer_counts_allowed(res.history, tol, res.its, ONCHIP_RTOL * res.history[0]) if res.converged else (res.its,)
    return Restated(osys.u0 + res.x, res.its, list(res.history), res.converged, stats, allowed)


@lru_cache(maxsize=None)
def exact_block_history(label, coeffs, preset):
    """Residual history of the same outer GMRES with sparse-LU block solves."""
    _, osys = system(label, coeffs)
    return list(o.gmres(osys.A, osys.rhs, o.fieldsplit_multiplicative_apply(osys.A, osys.n), **PRESETS[preset]).history)


@lru_cache(maxsize=None)
def direct_solution(label, coeffs):
    _, osys = system(label, coeffs)
    return o.solve_direct(osys)


def rel_max_error(x, u):
    m = float(np.abs(u).max())
    return float(np.abs(x - u).max()) / (m if m > 0.0 else 1.0)


def solution_bound(label, coeffs, preset):
    """10 x the restatement's own error against the direct solution (the factor covers the workgroup reduction's summation
    order), floor 1e-13."""
    return max(10.0 * rel_max_error(restated_solve(label, coeffs, preset).x, direct_solution(label, coeffs)), 1e-13)


def free_block_condition(Ab):
    """(kappa(S), kappa(D)) of the free rows of a block: S = D^-1/2 A D^-1/2.  Constrained rows are identity rows with zero
    columns and a zero right-hand side: they take no part in the solve."""
    Ab = sp.csr_matrix(Ab)
    d = Ab.diagonal()
    off = abs(Ab - sp.diags(d)).sum(axis=1).A1
    free = np.nonzero(~((off == 0.0) & (d == 1.0)))[0]
    if free.size == 0:
        return 1.0, 1.0
    Af = Ab[free][:, free].tocsc()
    df = Af.diagonal()
    s = sp.diags(1.0 / np.sqrt(df))
    S = (s @ Af @ s).tocsc()
    if free.size <= 400:
        ev = np.linalg.eigvalsh(S.toarray())
        lo, hi = ev[0], ev[-1]
    else:
        hi = spla.eigsh(S, k=1, which="LA", return_eigenvectors=False, tol=1e-8)[0]
        lo = spla.eigsh(S, k=1, sigma=0.0, which="LM", return_eigenvectors=False, tol=1e-8)[0]
    return float(hi / lo), float(df.max() / df.min())


def block_solve_bound(Ab, rtol=ONCHIP_RTOL):
    """||x - x*||_2 / ||x*||_2 of a solve that stopped on ||D^-1 r|| <= rtol ||D^-1 b||: with e = D^-1/2 S^-1 D^1/2 (D^-1 r)
    and D^-1 b = D^-1/2 S D^1/2 x*,  ||e|| <= rtol kappa(S) kappa(D) ||x*||.  The recurrence residual follows the true one,
    and the sparse direct solve its own solution, to a modest multiple of the unit roundoff times the same condition
    number: 100 eps is added to rtol for both."""
    ks, kd = free_block_condition(Ab)
    return (rtol + 100.0 * np.finfo(np.float64).eps) * ks * kd
