"""NumPy / SciPy restatement of the adjoint quantities, written from their definitions and independent of the library's
kernels.  The reference project computes no sensitivities: this is the yardstick, and tests/test_adjoint_host.py pins it
against central finite differences of its own direct solve.

K and M come from tests/flux_reference.py (Gauss quadrature on every cell's own affine map), boundary nodes from its
boundary_nodes.  With a = k1 / mu, b = beta / mu, c = k2 / mu the un-eliminated operator is

  A = [[a K + b M, -b M], [-b M, c K + b M]]

p: the full solution, Dirichlet values included; free rows: A_ff p_f = -A_fc g.  J a functional of p, gJ = dJ/dp.
lambda: A_ff lambda_f = gJ_f, lambda_c = 0.  Then

  o0 = lambda1^T K p1,  o1 = lambda2^T K p2,  o2 = (lambda1 - lambda2)^T M (p1 - p2)
  dJ/dk1 = -o0 / mu,  dJ/dk2 = -o1 / mu,  dJ/dbeta = -o2 / mu,  dJ/dmu = (k1 o0 + k2 o1 + beta o2) / mu^2
  dJ/dg_d = gJ_d - (A lambda)_d on the constrained dofs d

Every term comes with the sum of the absolute values of the products that were added: the scale of the rounding error of
any order of summation.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import flux_reference as FR

QUAD, TRI, HEX, TET = FR.QUAD, FR.TRI, FR.HEX, FR.TET
NAMES = {QUAD: "quad", TRI: "tri", HEX: "hex", TET: "tet"}

# (kind, degree, nx, ny, nz): the small cases of the finite-difference check; the first, third and (at degree 1) the others'
# meshes are what the GPU tests solve on
FD_CASES = [(QUAD, 1, 5, 3, 0), (TRI, 2, 4, 3, 0), (HEX, 1, 3, 4, 2), (TET, 2, 2, 3, 2)]
PARAM_SETS = [(1.0, 0.01, 1.0, 1.0), (1.0, 0.01, 3.0, 2.0), (1.0, 1e-4, 100.0, 1.0)]


def operator(sp_: FR.Space, k1, k2, beta, mu) -> sp.csr_matrix:
    """The un-eliminated 2n x 2n operator, field-major."""
    K, M = FR.stiffness_mass(sp_)
    a, b, c = k1 / mu, beta / mu, k2 / mu
    return sp.bmat([[a * K + b * M, -b * M], [-b * M, c * K + b * M]], format="csr")


def constrained_dofs(sp_: FR.Space) -> np.ndarray:
    bnd = FR.boundary_nodes(sp_)
    return np.concatenate([bnd, sp_.n + bnd])


def free_dofs(sp_: FR.Space) -> np.ndarray:
    return np.setdiff1d(np.arange(2 * sp_.n), constrained_dofs(sp_))


def _direct(Aff, rhs):
    return spla.spsolve(Aff.tocsc(), rhs)


def forward(sp_: FR.Space, k1, k2, beta, mu, g, solve=_direct) -> np.ndarray:
    """p (2n, field-major) with p = g on the constrained dofs (g: 2n values, read there only) and A p = 0 on the free rows."""
    A = operator(sp_, k1, k2, beta, mu)
    cd, fr = constrained_dofs(sp_), free_dofs(sp_)
    p = np.zeros(2 * sp_.n)
    p[cd] = np.asarray(g, dtype=np.float64)[cd]
    p[fr] = solve(A[fr][:, fr], -(A[fr][:, cd] @ p[cd]))
    return p


def solve_free(sp_: FR.Space, k1, k2, beta, mu, b, solve=_direct) -> np.ndarray:
    """x with F A F x = F b, 0 on the constrained dofs (what pph_solve_rhs returns)."""
    A = operator(sp_, k1, k2, beta, mu)
    fr = free_dofs(sp_)
    x = np.zeros(2 * sp_.n)
    x[fr] = solve(A[fr][:, fr], np.asarray(b, dtype=np.float64)[fr])
    return x


def _form(Mx: sp.csr_matrix, u, v):
    """(u^T Mx v, sum of |u_i Mx_ij v_j|)."""
    C = Mx.tocoo()
    t = u[C.row] * C.data * v[C.col]
    return float(t.sum()), float(np.abs(t).sum())


def bilinear(sp_: FR.Space, lam, p):
    """((o0, o1, o2), (their sums of absolute values))."""
    K, M = FR.stiffness_mass(sp_)
    n = sp_.n
    lam, p = np.asarray(lam, dtype=np.float64), np.asarray(p, dtype=np.float64)
    r = [_form(K, lam[:n], p[:n]), _form(K, lam[n:], p[n:]), _form(M, lam[:n] - lam[n:], p[:n] - p[n:])]
    return tuple(x[0] for x in r), tuple(x[1] for x in r)


@dataclass
class Adjoint:
    lam: np.ndarray          # 2n, 0 on the constrained dofs
    terms: tuple             # (o0, o1, o2)
    abs_terms: tuple         # sums of the absolute values of the products added
    k1: float
    k2: float
    beta: float
    mu: float
    bcs: np.ndarray          # 2n: gJ_d - (A lambda)_d on the constrained dofs, 0 elsewhere


def sensitivities(sp_: FR.Space, k1, k2, beta, mu, p, gJ, solve=_direct) -> Adjoint:
    A = operator(sp_, k1, k2, beta, mu)
    gJ = np.asarray(gJ, dtype=np.float64)
    lam = solve_free(sp_, k1, k2, beta, mu, gJ, solve)
    terms, absn = bilinear(sp_, lam, p)
    o0, o1, o2 = terms
    cd = constrained_dofs(sp_)
    bc = np.zeros(2 * sp_.n)
    bc[cd] = gJ[cd] - (A @ lam)[cd]
    return Adjoint(lam, terms, absn, -o0 / mu, -o1 / mu, -o2 / mu, (k1 * o0 + k2 * o1 + beta * o2) / mu ** 2, bc)


# ---- the test functional and data shared by the host and the GPU tests ------------------------------------------------
def smooth_boundary_data(sp_: FR.Space) -> np.ndarray:
    """2n nodal values of two smooth fields (read on the boundary nodes only)."""
    X = sp_.coords
    x, y = X[:, 0], X[:, 1]
    z = X[:, 2] if sp_.dim == 3 else np.zeros_like(x)
    g1 = 1.0 + np.sin(1.3 * x + 0.4) * np.cos(0.9 * y) + 0.5 * z * z
    g2 = 0.3 + np.exp(-0.7 * x) * (1.0 + 0.6 * y) - 0.4 * np.sin(1.1 * z + 0.2)
    return np.concatenate([g1, g2])


def functional_data(sp_: FR.Space, seed: int):
    """(w, d) of J = 1/2 sum_i w_i (p_i - d_i)^2 over all 2n dofs, boundary dofs included."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, 2 * sp_.n), rng.uniform(-1.0, 1.0, 2 * sp_.n)


def J_of(p, w, d) -> float:
    return 0.5 * float(np.sum(w * (p - d) ** 2))


def dJ_of(p, w, d) -> np.ndarray:
    return w * (p - d)
