"""NumPy / SciPy restatement of the p-multigrid block preconditioner ``pph_pmg`` (test infrastructure only).

One symmetric V-cycle whose top level is the degree-2 operator (``p2_restatement``) and whose lower levels are the CG-1
geometric hierarchy on the same cells (``oracle.dpp_mg_oracle.build_hierarchy``):

    steps Chebyshev-Jacobi steps on the degree-2 level on [lam / 4, lam]  (zero guess),
    restrict the residual, one V-cycle of the CG-1 hierarchy, prolong the correction,
    steps Chebyshev-Jacobi steps again.

The degree-2 nodes are the lattice refined once, so a degree-2 dof on nx cells sits where a CG-1 dof on 2 nx cells sits,
and the value of a CG-1 function at a degree-2 node is multilinear interpolation (Q2) or the average over a cell edge
(P2 on left-diagonal triangles / Kuhn tetrahedra): the transfer between the two top levels is the h-transfer
``dpp_mg_oracle.prolongation`` with fine dims = the degree-2 lattice.  Where the cells cannot be coarsened (odd counts)
the CG-1 part is what the library's CG-1 cycle is on such a mesh: max(steps, 2) Chebyshev steps from a zero guess.
"""
from __future__ import annotations

import os
import sys
from typing import List

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import p2_restatement as R  # noqa: E402
from oracle import dpp_mg_oracle as G  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402


def lattice3(kind: int, nx: int, ny: int, nz: int):
    d = R.lattice_dims(kind, nx, ny, nz)
    return tuple(d) if len(d) == 3 else (d[0], d[1], 1)


def inject_mask(kind: int, nx: int, ny: int, nz: int, mask2: np.ndarray) -> np.ndarray:
    """Dirichlet mask of the CG-1 level: CG-1 node C <- degree-2 lattice point 2C."""
    px, py, pz = lattice3(kind, nx, ny, nz)
    m3 = np.asarray(mask2, bool).reshape(pz, py, px)
    return (m3[::2, ::2, ::2] if R.dim_of(kind) == 3 else m3[:, ::2, ::2]).ravel().copy()


def p_prolongation(kind: int, nx: int, ny: int, nz: int) -> sp.csr_matrix:
    """CG-1 on (nx, ny, nz) cells -> degree 2 on the same cells."""
    dim = R.dim_of(kind)
    return G.prolongation(kind, (nx + 1, ny + 1, (nz + 1) if dim == 3 else 1), lattice3(kind, nx, ny, nz))


def operator2(kind: int, nx: int, ny: int, nz: int, coefK: float, coefM: float) -> sp.csr_matrix:
    K, M = R.assemble_KM(kind, nx, ny, nz)
    return (coefK * K + coefM * M).tocsr()


def build_levels(kind: int, nx: int, ny: int, nz: int, coefK: float, coefM: float, mask2: np.ndarray) -> List[G.Level]:
    """[degree-2 level] + CG-1 hierarchy; mask2: True on the constrained degree-2 dofs."""
    dim = R.dim_of(kind)
    mask2 = np.asarray(mask2, bool)
    A = G.eliminate(operator2(kind, nx, ny, nz, coefK, coefM), mask2)
    d = A.diagonal()
    lam = float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() / d))
    top = G.Level(A, 1.0 / d, mask2.copy(), lam)
    top.P = p_prolongation(kind, nx, ny, nz)
    lower = G.build_hierarchy(dim, kind, nx, ny, nz if dim == 3 else 0, coefK, coefM, inject_mask(kind, nx, ny, nz, mask2))
    return [top] + lower


def cycle(levels: List[G.Level], b: np.ndarray, steps: int = 2) -> np.ndarray:
    """z = B b: one application of pph_pmg."""
    top, lower = levels[0], levels[1:]
    x = G.chebyshev(top, b, None, steps)
    r = b - top.A @ x
    r[top.mask] = 0.0
    bc = top.P.T @ r
    bc[lower[0].mask] = 0.0
    if len(lower) == 1:
        xc = G.chebyshev(lower[0], bc, None, max(steps, 2))
    else:
        xc = G.vcycle(lower, bc, steps)
    corr = top.P @ xc
    corr[top.mask] = 0.0
    return G.chebyshev(top, b, x + corr, steps)


def pcg_iterations(levels: List[G.Level], rhs: np.ndarray, steps: int = 2, rtol: float = 1e-8, atol: float = 1e-300,
                   max_it: int = 200):
    """CG on the top level preconditioned by the cycle; (iterations, solution)."""
    res = o.pcg(levels[0].A, rhs, lambda v: cycle(levels, v, steps), rtol=rtol, atol=atol, max_it=max_it)
    return res.its, res.x
