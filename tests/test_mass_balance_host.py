"""Mass balance without a GPU: the NumPy restatement (tests/flux_reference.py) checks itself, the header and the binding
list carry the six new entry points, every argument refusal comes before a context exists, and the committed fixture of
direct-versus-consistent outflow gaps is what the restatement gives on the oracle's direct solve."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flux_reference as FR  # noqa: E402
from oracle import dpp_oracle as o  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(FR.QUAD, 5, 3, 0), (FR.QUAD, 2, 2, 0), (FR.QUAD, 1, 3, 0), (FR.TRI, 5, 3, 0), (FR.TRI, 2, 2, 0), (FR.TRI, 1, 3, 0),
         (FR.HEX, 3, 4, 2), (FR.HEX, 2, 2, 2), (FR.TET, 3, 4, 2), (FR.TET, 2, 2, 2)]
KD = [(c, deg) for c in SMALL for deg in (1, 2)]
IDS = [f"{('quad', 'tri', 'hex', 'tet')[c[0]]}{c[1]}x{c[2]}x{c[3]}-deg{deg}" for c, deg in KD]
GOLDEN = os.path.join(ROOT, "tests", "golden", "mass_balance_gaps.json")


@pytest.mark.parametrize("case,deg", KD, ids=IDS)
def test_restatement_linear_field_has_the_closed_form_fluxes(case, deg):
    """p = a . x + c: F_s = -+ kappa a_d |side| (|side| = 1), int p = a . (1/2, ..) + c, to 1e-14 of kappa max|a|."""
    kind, nx, ny, nz = case
    s = FR.space(kind, deg, nx, ny, nz)
    a, c, kappa = np.array([1.5, -2.0, 0.75])[:s.dim], 0.3, 2.0
    u = s.coords @ a + c
    F, _ = FR.boundary_fluxes(s, u, kappa)
    want = np.array([(kappa if side % 2 == 0 else -kappa) * a[side // 2] for side in range(2 * s.dim)])
    assert np.abs(F - want).max() <= 1e-14 * kappa * np.abs(a).max()
    assert abs(FR.integrate(s, u)[0] - (a.sum() / 2 + c)) <= 1e-14 * (np.abs(a).sum() + c)


@pytest.mark.parametrize("kind", (FR.QUAD, FR.TRI, FR.HEX, FR.TET), ids=("quad", "tri", "hex", "tet"))
@pytest.mark.parametrize("deg", (1, 2))
def test_restatement_nodal_fluxes_sum_to_the_transfer(kind, deg):
    """1^T r1 = T = -1^T r2 for a random field on each (kind, degree) pair, to 1e-12 of the sum of the absolute terms."""
    nx, ny, nz = (5, 3, 0) if FR.dim_of(kind) == 2 else (3, 4, 2)
    s = FR.space(kind, deg, nx, ny, nz)
    p = np.random.default_rng(7 + 2 * kind + deg).standard_normal(2 * s.n)
    k1, k2, beta, mu = 1.0, 0.01, 3.0, 2.0
    r = FR.nodal_fluxes(s, p, k1, k2, beta, mu)
    (i1, a1), (i2, a2) = FR.integrate(s, p[:s.n]), FR.integrate(s, p[s.n:])
    T = beta / mu * (i1 - i2)
    tol = 1e-12 * (beta / mu * (a1 + a2) + np.abs(r).sum())
    assert abs(r[:s.n].sum() - T) <= tol and abs(r[s.n:].sum() + T) <= tol
    b = FR.mass_balance(s, p, k1, k2, beta, mu)
    # the imbalance is the sum of the interior fluxes
    assert b.transfer == T and all(abs(b.imbalance[f]) <= b.interior_l1[f] + tol for f in (0, 1))


def test_new_entry_points_are_declared_and_bound():
    from perphil_amd import _ffi

    header = open(os.path.join(ROOT, "include", "perphil_hip.h")).read()
    for name in ("pph_integrate", "pph_integrate_device", "pph_boundary_flux", "pph_boundary_flux_device",
                 "pph_dpp_nodal_flux", "pph_dpp_nodal_flux_device"):
        assert name in _ffi.EXPORTS and f"int {name}(" in header and hasattr(_ffi.lib, name)


def test_argument_refusals_come_before_any_context():
    import perphil_amd as pa
    from perphil_amd import fd, postprocessing as pp

    params = pa.DPPParameters()
    for deg in (1, 2):
        mesh = fd.UnitSquareMesh(3, 2, quadrilateral=True, comm=fd.COMM_SELF)
        V = fd.FunctionSpace(mesh, "CG", deg)
        W = V * V
        p, w = fd.Function(V), fd.Function(W)
        vec = fd.Function(fd.VectorFunctionSpace(mesh, "CG", 1))
        for fn in (pp.mass_transfer_rate, pp.consistent_fluxes, pp.mass_balance):
            with pytest.raises(ValueError, match="2-field MixedFunctionSpace"):
                fn(p, params)
            with pytest.raises(ValueError, match="2-field MixedFunctionSpace"):
                fn(fd.Function(fd.MixedFunctionSpace([V, V, V])), params)
        # the two pressures on different lattices (a CG-1 and a degree-2 space): not one context's pair of fields
        other = fd.FunctionSpace(mesh, "CG", 3 - deg)
        for fn in (pp.mass_transfer_rate, pp.consistent_fluxes, pp.mass_balance):
            with pytest.raises(ValueError, match="same mesh"):
                fn(fd.Function(V * other), params)
        for f in (w, vec):
            with pytest.raises(ValueError, match="scalar CG space"):
                pp.integrate(f)
            with pytest.raises(ValueError, match="scalar CG space"):
                pp.boundary_fluxes(f, 1.0)
        for cond in (np.ones(V.dim()), fd.Function(V), lambda X: X[:, 0]):
            with pytest.raises(NotImplementedError, match="constant"):
                pp.boundary_fluxes(p, cond)
        assert mesh._ctx is None and not mesh.__dict__.get("_ctx_deg")


def _gap_case(n):
    """Direct minus consistent outflow of both networks on the oracle's direct solve: quadrilaterals n x n, degree 1,
    manufactured Dirichlet data, default parameters."""
    P = o.Params()
    m = o.build_mesh(2, o.CELL_QUAD, n, n)
    sysm = o.build_system(m, P)
    x = o.solve_direct(sysm)
    b = FR.mass_balance(FR.space(FR.QUAD, 1, n, n), x, P.k1, P.k2, P.beta, P.mu)
    return [float(b.outflow_direct[f].sum() - b.outflow_consistent[f]) for f in (0, 1)], b


def test_committed_gaps_are_the_restatement_on_the_direct_solve():
    """The gap is O(h): it is pinned by value, not by a threshold.  The fixture holds values only."""
    gold = json.load(open(GOLDEN))
    assert sorted(gold) == ["16", "32", "8"]
    prev = None
    for n in (8, 16, 32):
        gaps, b = _gap_case(n)
        scale = max(np.abs(b.outflow_direct[f]).sum() for f in (0, 1))
        assert np.abs(np.array(gaps) - np.array(gold[str(n)])).max() <= 1e-11 * scale
        # the direct solve leaves interior fluxes at rounding level: the imbalance is rounding
        for f in (0, 1):
            assert abs(b.imbalance[f]) <= b.interior_l1[f] + 1e-12 * b.scale
        if prev is not None:
            assert abs(gaps[0]) < abs(prev[0])      # shrinks with h
        prev = gaps
