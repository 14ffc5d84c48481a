"""NumPy restatement of the mass-balance quantities (boundary fluxes, volume integral, consistent nodal fluxes), written
from their definitions and independent of the library's kernels: where the kernels use closed-form integrals of the basis
on the uniform box, this file integrates by Gauss quadrature on every cell's own affine map, with gradients from the
inverse Jacobian of the cell's vertex coordinates.  The reference project computes no fluxes: this is the yardstick.

  F_s = int_{side s} -kappa grad(p_h) . n ds   sides 1: x = 0, 2: x = 1, 3: y = 0, 4: y = 1, 5: z = 0, 6: z = 1; n outward;
                                               the gradient of the cell that owns the facet
  I   = int p_h dx
  r1  = a K p1 + b M (p1 - p2),  r2 = c K p2 - b M (p1 - p2)   (a, b, c) = (k1, beta, k2) / mu, K and M without Dirichlet rows

Degree 1 takes meshes, K and M from the oracle; degree 2 from tests/p2_restatement.py.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass

import numpy as np

import p2_restatement as p2
from oracle import dpp_oracle as o

QUAD, TRI, HEX, TET = 0, 1, 2, 3


def dim_of(kind):
    return 2 if kind in (QUAD, TRI) else 3


@dataclass
class Space:
    kind: int
    degree: int
    nx: int
    ny: int
    nz: int
    coords: np.ndarray     # [n, dim]
    cells: np.ndarray      # [ncell, m]
    vertices: list         # local nodes that are the cell's vertices (tensor cells: corner bits order; simplices: 0 .. dim)

    @property
    def dim(self):
        return dim_of(self.kind)

    @property
    def n(self):
        return self.coords.shape[0]


_spaces = {}


def space(kind, degree, nx, ny, nz=0) -> Space:
    key = (kind, degree, nx, ny, nz)
    if key not in _spaces:
        d = dim_of(kind)
        if degree == 1:
            m = o.build_mesh(d, kind, nx, ny, nz)
            X, cells = m.coords, m.cells
            verts = list(range(cells.shape[1]))
        else:
            X, cells = p2.coords(kind, nx, ny, nz), p2.dofmap(kind, nx, ny, nz)
            if kind in (QUAD, HEX):   # corner (bx, by, bz) of the box is the local node 2 bx + 6 by + 18 bz
                verts = [2 * (v & 1) + 6 * ((v >> 1) & 1) + 18 * ((v >> 2) & 1) for v in range(1 << d)]
            else:
                verts = list(range(d + 1))
        _spaces[key] = Space(kind, degree, nx, ny, nz, X, cells, verts)
    return _spaces[key]


_km = {}


def stiffness_mass(sp_: Space):
    key = (sp_.kind, sp_.degree, sp_.nx, sp_.ny, sp_.nz)
    if key not in _km:
        if sp_.degree == 1:
            _km[key] = o.assemble_scalar(o.build_mesh(sp_.dim, sp_.kind, sp_.nx, sp_.ny, sp_.nz))
        else:
            _km[key] = p2.assemble_KM(sp_.kind, sp_.nx, sp_.ny, sp_.nz)
    return _km[key]


def basis(kind, degree, xi):
    """Values [m] and reference gradients [m, d] at the reference point xi (unit cube / unit simplex)."""
    if degree == 2:
        return p2.basis(kind, np.asarray(xi, dtype=float))
    d = dim_of(kind)
    xi = np.asarray(xi, dtype=float)
    if kind in (QUAD, HEX):
        N, G = np.ones(1 << d), np.ones((1 << d, d))
        for b in range(1 << d):
            for e in range(d):
                up = (b >> e) & 1
                N[b] *= xi[e] if up else 1 - xi[e]
                for f in range(d):
                    G[b, f] *= (1.0 if up else -1.0) if f == e else (xi[e] if up else 1 - xi[e])
        return N, G
    return np.concatenate([[1 - xi.sum()], xi]), np.vstack([-np.ones(d), np.eye(d)])


def _jacobians(sp_: Space):
    """J[c] (columns: the edges from vertex 0 to the vertices that span the affine map), its inverse, |det|."""
    V = sp_.coords[sp_.cells[:, sp_.vertices]]                      # [nc, nv, d]
    span = [1 << e for e in range(sp_.dim)] if sp_.kind in (QUAD, HEX) else list(range(1, sp_.dim + 1))
    J = np.transpose(V[:, span, :] - V[:, :1, :], (0, 2, 1))        # [nc, d(x), d(xi)]
    return V, J, np.linalg.inv(J), np.abs(np.linalg.det(J))


_G3 = (0.5 + 0.5 * np.polynomial.legendre.leggauss(3)[0], 0.5 * np.polynomial.legendre.leggauss(3)[1])


def _reference_facets(kind):
    """[(vertex positions of the facet among the cell's vertices, [(xi, weight)], weights summing to 1)]: 3-point Gauss
    per direction on edges / quadrilateral faces (degree 5), the 3-point interior rule on triangles (degree 2: the normal
    derivative of a P2 function is linear there)."""
    d = dim_of(kind)
    gx, gw = _G3
    out = []
    if kind in (QUAD, HEX):
        for e in range(d):
            for t in (0, 1):
                verts = [v for v in range(1 << d) if ((v >> e) & 1) == t]
                rule = []
                for idx in itertools.product(range(3), repeat=d - 1):
                    xi, k = np.zeros(d), 0
                    for f in range(d):
                        if f == e:
                            xi[f] = t
                        else:
                            xi[f] = gx[idx[k]]
                            k += 1
                    rule.append((xi, float(np.prod([gw[i] for i in idx]))))
                out.append((verts, rule))
        return out
    ref = np.vstack([np.zeros(d), np.eye(d)])      # reference vertices
    for opp in range(d + 1):
        verts = [r for r in range(d + 1) if r != opp]
        if d == 2:
            rule = [((1 - t) * ref[verts[0]] + t * ref[verts[1]], w) for t, w in zip(gx, gw)]
        else:
            rule = []
            for k in range(3):
                lam = np.full(3, 1.0 / 6.0)
                lam[k] = 2.0 / 3.0
                rule.append((lam @ ref[verts], 1.0 / 3.0))
        out.append((verts, rule))
    return out


def _measure(P):
    """Measure of the facets with vertices P [nf, nv, d]: a segment, a triangle or a parallelogram (vertices in the
    order of the corner bits)."""
    d = P.shape[2]
    if d == 2:
        return np.linalg.norm(P[:, 1] - P[:, 0], axis=1)
    c = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    return c if P.shape[1] == 4 else 0.5 * c


def boundary_fluxes(sp_: Space, u, kappa):
    """(F [2 dim], A [2 dim]): the side fluxes and, per side, the sum of the absolute values of the terms that were added
    (the scale of the rounding error of any summation order)."""
    u = np.asarray(u, dtype=np.float64)
    d = sp_.dim
    V, _, Ji, _ = _jacobians(sp_)
    U = u[sp_.cells]                                              # [nc, m]
    F, A = np.zeros(2 * d), np.zeros(2 * d)
    for verts, rule in _reference_facets(sp_.kind):
        P = V[:, verts, :]                                          # [nc, nfv, d]
        for side in range(2 * d):
            ax, val = side // 2, float(side % 2)
            on = np.all(P[:, :, ax] == val, axis=1)
            if not on.any():
                continue
            meas = _measure(P[on])
            sign = 1.0 if val == 1.0 else -1.0
            for xi, w in rule:
                _, G = basis(sp_.kind, sp_.degree, xi)              # [m, d] reference gradients
                gref = U[on] @ G                                    # [nf, d]: dp / dxi
                dpdn = sign * np.einsum("ce,ce->c", gref, Ji[on][:, :, ax])   # dp/dx_ax = sum_e dp/dxi_e dxi_e/dx_ax
                term = -kappa * w * meas * dpdn
                F[side] += term.sum()
                A[side] += np.abs(term).sum()
    return F, A


def integrate(sp_: Space, u):
    """(int p_h dx, sum of |terms|)."""
    u = np.asarray(u, dtype=np.float64)
    _, _, _, det = _jacobians(sp_)
    pts, wts = p2.reference_rule(sp_.kind, 4)
    wN = sum(w * basis(sp_.kind, sp_.degree, xi)[0] for xi, w in zip(pts, wts))   # int N_b over the reference cell
    terms = det[:, None] * u[sp_.cells] * wN[None, :]
    return float(terms.sum()), float(np.abs(terms).sum())


def nodal_fluxes(sp_: Space, p, k1, k2, beta, mu):
    """r = (r1, r2), field-major."""
    K, M = stiffness_mass(sp_)
    n = sp_.n
    p = np.asarray(p, dtype=np.float64)
    p1, p2_ = p[:n], p[n:]
    m = M @ (p1 - p2_)
    return np.concatenate([(k1 / mu) * (K @ p1) + (beta / mu) * m, (k2 / mu) * (K @ p2_) - (beta / mu) * m])


def boundary_nodes(sp_: Space):
    X = sp_.coords
    return np.nonzero(np.any((X == 0.0) | (X == 1.0), axis=1))[0].astype(np.int64)


@dataclass
class Balance:
    transfer: float
    outflow_consistent: tuple
    outflow_direct: tuple      # two arrays [2 dim]
    imbalance: tuple
    r: np.ndarray
    interior_l1: tuple         # 1-norms of the interior entries of r1, r2
    scale: float               # sum of the absolute values of everything the imbalance adds up


def mass_balance(sp_: Space, p, k1, k2, beta, mu) -> Balance:
    n = sp_.n
    p = np.asarray(p, dtype=np.float64)
    i1, a1 = integrate(sp_, p[:n])
    i2, a2 = integrate(sp_, p[n:])
    T = beta / mu * (i1 - i2)
    r = nodal_fluxes(sp_, p, k1, k2, beta, mu)
    b = boundary_nodes(sp_)
    inner = np.setdiff1d(np.arange(n), b)
    out = (-r[b].sum(), -r[n + b].sum())
    direct = (boundary_fluxes(sp_, p[:n], k1 / mu)[0], boundary_fluxes(sp_, p[n:], k2 / mu)[0])
    scale = beta / mu * (a1 + a2) + np.abs(r).sum()
    return Balance(T, out, direct, (out[0] + T, out[1] - T), r,
                   (np.abs(r[inner]).sum(), np.abs(r[n + inner]).sum()), scale)
