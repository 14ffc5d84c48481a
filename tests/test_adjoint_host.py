"""Adjoint solves and sensitivities without a GPU: the NumPy restatement (tests/adjoint_reference.py) is pinned against
central finite differences of its own direct solve, so that the GPU tests can stand on it; the header, the binding list and
the library carry the four entry points; every Python refusal comes before a context exists."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adjoint_reference as AR  # noqa: E402
import flux_reference as FR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{AR.NAMES[c[0]]}{c[2]}x{c[3]}x{c[4]}-deg{c[1]}" for c in AR.FD_CASES]
PIDS = ["k2=1e-2,beta=1,mu=1", "k2=1e-2,beta=3,mu=2", "k2=1e-4,beta=100,mu=1"]


LD = np.longdouble


class _Extended:
    """The restatement's formulas once more in longdouble, for the comparison with difference quotients only: the operator
    a K + b M formed in longdouble from the restatement's K and M, its direct solve (the LU factors of the float64 operator)
    refined three times on the longdouble residual, sums in longdouble.  In float64 the entries of k2 K + beta M carry a
    rounding of about eps beta M, which for (k2, beta) = (1e-4, 100) is a noise of 1e-11 in k2 itself: a difference quotient
    at the relative step 5e-4 cannot be read below 1e-8 through it, and its truncation error in k2 is 1e-10 there."""

    def __init__(self, sp_):
        K, M = FR.stiffness_mass(sp_)
        self.sp, self.n = sp_, sp_.n
        self.K, self.M = K.toarray().astype(LD), M.toarray().astype(LD)
        self.cd, self.fr = AR.constrained_dofs(sp_), AR.free_dofs(sp_)

    def operator(self, k1, k2, beta, mu):
        a, b, c = LD(k1) / LD(mu), LD(beta) / LD(mu), LD(k2) / LD(mu)
        return np.block([[a * self.K + b * self.M, -b * self.M], [-b * self.M, c * self.K + b * self.M]])

    def _solve(self, A, rhs):
        fr = self.fr
        Aff = A[np.ix_(fr, fr)]
        lu = spla.splu(sp.csc_matrix(Aff.astype(np.float64)))
        x = lu.solve(rhs.astype(np.float64)).astype(LD)
        for _ in range(3):
            x = x + lu.solve((rhs - Aff @ x).astype(np.float64)).astype(LD)
        return x

    def forward(self, params, g):
        A = self.operator(*params)
        p = np.zeros(2 * self.n, dtype=LD)
        p[self.cd] = np.asarray(g)[self.cd]
        p[self.fr] = self._solve(A, -(A[np.ix_(self.fr, self.cd)] @ p[self.cd]))
        return p

    def sensitivities(self, params, p, gJ):
        k1, k2, beta, mu = (LD(v) for v in params)
        n = self.n
        A = self.operator(*params)
        lam = np.zeros(2 * n, dtype=LD)
        lam[self.fr] = self._solve(A, gJ[self.fr])
        o0, o1 = lam[:n] @ (self.K @ p[:n]), lam[n:] @ (self.K @ p[n:])
        o2 = (lam[:n] - lam[n:]) @ (self.M @ (p[:n] - p[n:]))
        bc = np.zeros(2 * n, dtype=LD)
        bc[self.cd] = gJ[self.cd] - (A @ lam)[self.cd]
        return dict(k1=-o0 / mu, k2=-o1 / mu, beta=-o2 / mu, mu=(k1 * o0 + k2 * o1 + beta * o2) / mu ** 2, terms=(o0, o1, o2),
                    bcs=bc, lam=lam)


@pytest.mark.parametrize("params", AR.PARAM_SETS, ids=PIDS)
@pytest.mark.parametrize("case", AR.FD_CASES, ids=IDS)
def test_restatement_against_central_differences(case, params):
    """dJ/dk1, dJ/dk2, dJ/dbeta against central differences at the relative steps 1e-3 and 5e-4: at most 1e-5 at 1e-3 (8 x
    the truncation error measured for these cases) and a ratio in [3, 5] between the two steps (pure truncation: 4 per
    halving) - wherever the discrepancy is large enough to be resolved at all: for (k2, beta) = (1e-4, 100) J is linear in k2
    to 1e-12, the discrepancy in dJ/dk2 is then the noise of the quotient itself, and no ratio is asserted below the
    resolution computed in the test.  dJ/dmu is lam^T A p: at most 1e-10 of its terms' scale, and so is the finite difference of J in mu.  Boundary
    data: a directional derivative at step 1e-4, at most 1e-8 (J is quadratic in the data: no truncation error).  These
    comparisons run on the formulas in longdouble (_Extended says why); the restatement itself (float64, spsolve) then has
    to give the same three terms, adjoint and boundary gradient to 1e-10 - of the sums of the absolute values of the terms'
    products, of the largest entry - the bar the GPU tests start from, and its own dJ/dmu has to meet the same bound."""
    kind, deg, nx, ny, nz = case
    sp_ = FR.space(kind, deg, nx, ny, nz)
    g = AR.smooth_boundary_data(sp_)
    w, d = AR.functional_data(sp_, 11)
    X = _Extended(sp_)
    p = X.forward(params, g)
    ad = X.sensitivities(params, p, w * (p - d))

    def J_diff(q_up, q_dn, g_up=g, g_dn=g):
        # J(up) - J(dn) = 1/2 sum w (p_up - p_dn)(p_up + p_dn - 2 d): the same number without the cancellation of two J's
        pu, pd = X.forward(q_up, g_up), X.forward(q_dn, g_dn)
        return 0.5 * np.sum(w * (pu - pd) * (pu + pd - 2.0 * d))

    # What a quotient at the half step resolves: the refined solves leave about eps cond(A_ff) |p| in p (longdouble eps), that
    # is sum |dJ/dp_i| |p_i| eps cond in J, against the quotient's numerator 2 h theta dJ/dtheta.  Two decimal digits above
    # that a ratio can be read.
    Aff = AR.operator(sp_, *params)[X.fr][:, X.fr].toarray()
    dJ_noise = float(np.sum(np.abs(w * (p - d)) * np.abs(p))) * float(np.finfo(LD).eps) * float(np.linalg.cond(Aff))
    for i, name in enumerate(("k1", "k2", "beta")):
        floor = 100.0 * dJ_noise / (2.0 * 5e-4 * abs(params[i] * float(ad[name])))
        err = []
        for h in (1e-3, 5e-4):
            up, dn = list(params), list(params)
            up[i] *= 1.0 + h
            dn[i] *= 1.0 - h
            fdiff = J_diff(up, dn) / (LD(up[i]) - LD(dn[i]))
            err.append(float(abs(fdiff - ad[name]) / abs(ad[name])))
        print(f"{name}: dJ = {float(ad[name]):.6e}, relative discrepancy {err[0]:.2e} (1e-3), {err[1]:.2e} (5e-4), "
              f"ratio {err[0] / err[1]:.2f}")
        assert err[0] <= 1e-5
        if err[0] >= floor:
            assert 3.0 <= err[0] / err[1] <= 5.0
        else:
            print(f"   (below {floor:.1e}: no ratio can be read)")
    k1, k2, beta, mu = params
    o0, o1, o2 = (float(o) for o in ad["terms"])
    scale = (abs(k1 * o0) + abs(k2 * o1) + abs(beta * o2)) / mu ** 2
    h = 1e-3
    fd_mu = float(J_diff((k1, k2, beta, mu * (1 + h)), (k1, k2, beta, mu * (1 - h))) / (2 * h * mu))
    print(f"mu: dJ = {float(ad['mu']):.2e}, finite difference {fd_mu:.2e}, scale {scale:.2e}")
    assert abs(ad["mu"]) <= 1e-10 * scale
    assert abs(fd_mu) <= 1e-10 * scale
    # boundary data
    rng = np.random.default_rng(5)
    cd = AR.constrained_dofs(sp_)
    dg = np.zeros(2 * sp_.n)
    dg[cd] = rng.uniform(-1.0, 1.0, cd.size)
    h = 1e-4
    fd_g = J_diff(params, params, g + h * dg, g - h * dg) / (2 * h)
    an = ad["bcs"] @ dg
    print(f"boundary direction: {float(an):.6e}, relative discrepancy {float(abs(fd_g - an) / abs(an)):.2e}")
    assert abs(fd_g - an) <= 1e-8 * abs(an)
    # the restatement itself
    p0 = AR.forward(sp_, *params, g)
    ad0 = AR.sensitivities(sp_, *params, p0, AR.dJ_of(p0, w, d))
    loss = max(float(abs(a - b)) / s_ for a, b, s_ in zip(ad0.terms, ad["terms"], ad0.abs_terms))
    loss_lam = float(np.abs(ad0.lam - ad["lam"]).max() / np.abs(ad["lam"]).max())
    loss_bc = float(np.abs(ad0.bcs - ad["bcs"]).max() / np.abs(ad["bcs"]).max())
    print(f"float64 restatement: terms {loss:.2e} of their absolute sums, adjoint {loss_lam:.2e}, boundary gradient "
          f"{loss_bc:.2e} of the largest entry, dJ/dmu {ad0.mu:.2e}")
    assert loss <= 1e-10 and loss_lam <= 1e-10 and loss_bc <= 1e-10
    assert abs(ad0.mu) <= 1e-10 * scale
    assert np.all(ad0.bcs[AR.free_dofs(sp_)] == 0.0) and np.all(ad0.lam[cd] == 0.0)


def test_entry_points_are_declared_and_bound():
    from perphil_amd import _ffi

    header = open(os.path.join(ROOT, "include", "perphil_hip.h")).read()
    for name in ("pph_solve_rhs", "pph_solve_rhs_device", "pph_dpp_bilinear", "pph_dpp_bilinear_device"):
        assert name in _ffi.EXPORTS and f"int {name}(" in header and hasattr(_ffi.lib, name)
    for name in ("solve_rhs", "dpp_bilinear"):
        assert callable(getattr(_ffi.Context, name))


def test_refusals_come_before_any_context():
    import torch

    from perphil_amd import DPPParameters, adjoint, fd
    from perphil_amd.partition import make_slab
    from perphil_amd.solver_parameters import LINEAR_SOLVER_PARAMS

    P = DPPParameters(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
    mesh = fd.UnitSquareMesh(3, 2, quadrilateral=True, comm=fd.COMM_SELF)
    V1, V2 = fd.FunctionSpace(mesh, "CG", 1), fd.FunctionSpace(mesh, "CG", 2)
    W1, W2 = V1 * V1, V2 * V2
    n2 = W1.dim()
    bcs = [fd.DirichletBC(W1.sub(0), 1.0), fd.DirichletBC(W1.sub(1), 0.0)]
    ilu = {"ksp_type": "gmres", "pc_type": "ilu", "ksp_rtol": 1e-12}
    good = np.zeros(n2)
    # wrong length or dtype of the right-hand side / of dJ_dp / of the solution
    for bad in (np.zeros(n2 + 1), np.zeros(n2, dtype=np.float32), np.zeros((n2, 1)), torch.zeros(n2, dtype=torch.float32),
                torch.zeros(n2 - 1, dtype=torch.float64), fd.Function(V1), fd.Function(W2)):
        with pytest.raises(ValueError):
            adjoint.adjoint_solve(W1, P, bcs, bad, ilu)
        with pytest.raises(ValueError):
            adjoint.sensitivities(W1, P, bcs, good, bad, ilu)
        with pytest.raises(ValueError):
            adjoint.sensitivities(W1, P, bcs, bad, good, ilu)
    # not a 2-field mixed space
    with pytest.raises(ValueError, match="2-field"):
        adjoint.adjoint_solve(V1, P, bcs, good, ilu)
    # degree 2: the option refusals of solve_dpp
    bcs2 = [fd.DirichletBC(W2.sub(0), 1.0), fd.DirichletBC(W2.sub(1), 0.0)]
    for opts in (LINEAR_SOLVER_PARAMS, {"ksp_type": "cg", "pc_type": "pph_cmg"}):
        with pytest.raises(NotImplementedError, match="degree-2"):
            adjoint.adjoint_solve(W2, P, bcs2, np.zeros(W2.dim()), opts)
        with pytest.raises(NotImplementedError, match="degree-2"):
            adjoint.sensitivities(W2, P, bcs2, np.zeros(W2.dim()), np.zeros(W2.dim()), opts)
    with pytest.raises(NotImplementedError):
        adjoint.adjoint_solve(W1, P, bcs, good, {"ksp_type": "bcgs"})
    assert mesh._ctx is None and not mesh.__dict__.get("_ctx_deg")
    # a distributed mesh (the slab of rank 0 of 2, set by hand: no process group in this test)
    cube = fd.UnitCubeMesh(2, 2, 4, hexahedral=True, comm=fd.COMM_SELF)
    Vc = fd.FunctionSpace(cube, "CG", 1)
    Wc = Vc * Vc
    cube._slab = make_slab(2, 2, 4, 2, 0)
    assert cube.distributed
    bc_c = [fd.DirichletBC(Wc.sub(0), 1.0), fd.DirichletBC(Wc.sub(1), 0.0)]
    z = np.zeros(Wc.local_dim())
    with pytest.raises(NotImplementedError, match="comm=fd.COMM_SELF"):
        adjoint.adjoint_solve(Wc, P, bc_c, z, ilu)
    with pytest.raises(NotImplementedError, match="comm=fd.COMM_SELF"):
        adjoint.sensitivities(Wc, P, bc_c, z, z, ilu)
    assert cube._ctx is None
    # the frozen result class
    s = adjoint.Sensitivities(k1=1.0, k2=2.0, beta=3.0, mu=0.0, terms=(1.0, 2.0, 3.0), adjoint=fd.Function(W1))
    assert s.bcs is None and s.info == {}
    with pytest.raises(Exception):
        s.k1 = 2.0
