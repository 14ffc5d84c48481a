"""The CG-1 kernels of pph_post.hip past their launch caps, against tests/post_reference.py (pinned on the CPU by
test_post_scale_host.py).  Every case asserts the branch it is meant to take from the launch rules restated in
post_reference.py (norm kernels: min(ceil(cells / 256), 2048) workgroups, a second cell per thread past 524 288 cells;
projection: min(ceil(n / 256), 8192), a second node per thread past 2 097 152 nodes) and prints mesh, size, passes per
thread, worst error and bound.  Large contexts are closed at the end of each test.

Bounds - derived, nothing tuned to the device.

Error norms.  delta = relative discrepancy of the fp64 reference sum from the same reference evaluated in np.longdouble;
a device sum S must satisfy |S - S_ref| <= max(100 delta, 1e-13) S_ref (the convention of the ILU(0) cases in
tests/README.md).  delta is computed per case, per nodal field and per sum; for the plain interpolant (u_h - p of order
h^2) it is orders larger than for the perturbed one: that is the cancellation in u_h - p, not slack.  Quadrature points:
2 (nb + 3 d + 2) u max |x| elementwise (post_reference.points_bound).

Darcy projection.  darcy() solves M u_d = b_d by pph_cg_jacobi(rtol 1e-13, atol 0, max_it 1000) (pph_post.hip:986), which
calls cg_solve with norm_type 0 (pph_solve.hip:448), the preconditioned-norm loop: z = dinv .* r and res = sqrt(z.z)
(pph_solve.hip:400-404), bnorm = res of the zero guess = ||D^-1 b||_2 (:405), tol = max(rtol * bnorm, atol) (:407), and
"if (res <= tol) converged" after every update (:435; :411 for the guess).  It stops at ||D^-1 r||_2 <= 1e-13 ||D^-1 b||_2.  The test evaluates
r = b_ref - M u with the matrix-free reference and asserts

    ||D^-1 r||_2 <= (1e-13 + 100 drift) ||D^-1 b_ref||_2,

drift = the reference's own residual-evaluation drift, fp64 against np.longdouble, measured on a small mesh of the same
cell kind (post_reference.residual_drift; it also covers the rounding of the device's right-hand side).  With
S = D^-1/2 M D^-1/2 (same spectrum as D^-1 M), u - M^-1 b = M^-1 r = D^-1/2 S^-1 D^1/2 (D^-1 r), hence

    ||u - M^-1 b||_2 <= sqrt(max D / min D) / lambda_min(D^-1 M) ||D^-1 r||_2,

lambda_min >= 1/2 (P1 simplices), 1/4 (Q1 quadrilaterals), 1/8 (Q1 hexahedra) by Wathen's element-wise bounds, max D /
min D computed from the reference's diagonal and printed (uniform box: 4, 6, 8, 12 away from degenerate sizes).  That bounds
the distance from the constant -k a (linear pressure: M^-1 b exactly) and, together with the same bound applied to the
direct solve's own residual, the distance from the direct solve (Kronecker solve on quadrilaterals and hexahedra at scale,
the oracle's sparse LU on the small meshes).  A projection that ran into max_it would fail the residual assertion."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import post_reference as PR  # noqa: E402

from oracle import dpp_oracle as o  # noqa: E402
from perphil_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu

assert (_ffi.CELL_QUAD, _ffi.CELL_TRI, _ffi.CELL_HEX, _ffi.CELL_TET) == (PR.QUAD, PR.TRI, PR.HEX, PR.TET)
K1, K2, BETA, MU = PR.K1, PR.K2, PR.BETA, PR.MU


def _ctx(gpu_ctx_factory, case):
    kind, nx, ny, nz = case
    ctx = gpu_ctx_factory()
    ctx.mesh_build(PR.dim_of(kind), kind, nx, ny, nz)
    assert ctx.ncell == PR.n_cells(*case) and ctx.n == PR.n_nodes(*case)
    return ctx


class _Field0:
    """the first manufactured pressure and its gradient as the callables of error_norms_sampled; one evaluation (on the
    thread pool) serves both calls on the same point array"""

    def __init__(self, ex):
        def both(Y):
            P, G = ex(Y)
            return np.column_stack([P[0], G[0]])

        self._both, self._X, self._v = PR.threaded(both), None, None

    def _eval(self, X):
        if self._X is not X:
            self._X, self._v = X, self._both(X)
        return self._v

    def value(self, X):
        return self._eval(X)[:, 0]

    def grad(self, X):
        return self._eval(X)[:, 1:]


def _norm_case(gpu_ctx_factory, name, case, nqs, passes_expected, chunks):
    import torch

    kind = case[0]
    ctx = _ctx(gpu_ctx_factory, case)
    try:
        cells, X = ctx.dofmap(), ctx.coords()
        nc = ctx.ncell
        grid, passes = PR.norm_launch(nc)
        assert passes == passes_expected and (grid == PR.NORM_GRID_CAP) == (nc >= PR.NORM_LANES)
        for nq in nqs:
            ref = PR.norm_reference(kind, cells, X, nq)
            print(f"{name} nq {nq}: {nc} cells, {grid} workgroups, {passes} pass(es) per thread "
                  f"({max(nc - PR.NORM_LANES, 0)} cells in the second); delta L2 {ref['delta']['l2']}, H1 {ref['delta']['h1']}")
            worst = np.zeros((4, 3))                          # per nodal field: fraction of the bound, relative L2^2, H1^2 error

            def check(tag, k, l2, h1):
                e = PR.norms_excess(ref, k, l2 * l2, h1 * h1)
                rel = (abs(l2 * l2 - ref["l2"][k]) / ref["l2"][k], abs(h1 * h1 - ref["h1"][k]) / ref["h1"][k])
                worst[k] = np.maximum(worst[k], (e,) + rel)
                assert e <= 1.0, (f"{name} nq {nq} {tag} {PR.NODAL_NAME[k]}: L2^2 {l2 * l2!r} vs {ref['l2'][k]!r} (bound "
                                  f"{ref['bound']['l2'][k]:.2e}), H1^2 {h1 * h1!r} vs {ref['h1'][k]!r} (bound {ref['bound']['h1'][k]:.2e})")

            for k in range(4):
                f, nodal = int(ref["fields"][k]), ref["nodal"][k]
                check("error_norms_mms", k, *ctx.error_norms_mms(f, nodal, K1, K2, BETA, MU, nq=nq))
                t = torch.as_tensor(nodal, device=f"cuda:{ctx.device}")
                check("error_norms_mms_device", k, *ctx.error_norms_mms_device(f, t, K1, K2, BETA, MU, nq=nq))
            f0 = _Field0(ref["exact"])
            for k in (0, 2):                                   # the two nodal fields that go with the first pressure
                nodal = ref["nodal"][k]
                t = torch.as_tensor(nodal, device=f"cuda:{ctx.device}")
                for ch in chunks:
                    check(f"error_norms_sampled chunk {ch}", k,
                          *ctx.error_norms_sampled(nodal, f0.value, f0.grad, nq=nq, chunk_cells=ch))
                    check(f"error_norms_sampled_device chunk {ch}", k,
                          *ctx.error_norms_sampled_device(t, f0.value, f0.grad, nq=nq, chunk_cells=ch))
            for k in range(4):
                print(f"  {PR.NODAL_NAME[k]}: worst relative error of L2^2 {worst[k, 1]:.2e} (bound {ref['bound']['l2'][k]:.2e}), "
                      f"of H1^2 {worst[k, 2]:.2e} (bound {ref['bound']['h1'][k]:.2e}); {worst[k, 0]:.2e} of the bound")
            c0 = (nc - PR.NORM_LANES) // 2 if nc > PR.NORM_LANES else min(3, nc - 1)
            count = nc - c0
            if nc > PR.NORM_LANES:
                assert c0 > 0 and PR.norm_launch(count)[1] == 2
            xq = ctx.quadrature_points(nq, c0, count)
            xref = PR.quadrature_points(kind, cells, X, nq, (c0, c0 + count))
            e = PR.points_excess(kind, xq, xref)
            print(f"  quadrature points of cells [{c0}, {c0 + count}): max |x - x_ref| = {np.abs(xq - xref).max():.2e} "
                  f"(bound {PR.points_bound(kind, float(np.abs(xref).max())):.2e})")
            assert e <= 1.0
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(PR.NORM_PAST))
def test_error_norms_past_the_launch_cap(gpu_ctx_factory, name):
    """second pass of the grid-stride loop, all 2048 partial-sum slots live; sampled mode with a chunk larger than the cap
    (the second chunk starts at a large c0) and a small one that does not divide the cell count"""
    nc = PR.n_cells(*PR.NORM_PAST[name])
    big, small = (nc + PR.NORM_LANES) // 2 + 1, 100003
    assert PR.NORM_LANES < big < nc and nc % small and nc % big
    _norm_case(gpu_ctx_factory, name, PR.NORM_PAST[name], (3,), 2, (big, small))


def test_error_norms_at_the_launch_cap(gpu_ctx_factory):
    """exactly 524 288 cells: 2048 workgroups, no second pass"""
    (name, case), = PR.NORM_AT.items()
    _norm_case(gpu_ctx_factory, name, case, (3,), 1, (PR.n_cells(*case), 100003))


@pytest.mark.parametrize("name", list(PR.NORM_SMALL))
def test_error_norms_small_with_one_and_eight_points(gpu_ctx_factory, name):
    """below the cap, nq = 1 and 8 (GaussRule holds 8 points), chunks of 7 cells and one chunk"""
    case = PR.NORM_SMALL[name]
    _norm_case(gpu_ctx_factory, name, case, (1, 8), 1, (7, PR.n_cells(*case)))


_DRIFT = {}


def _drift(kind):
    """the reference's residual-evaluation drift on the small mesh of this cell kind, at the oracle's projection"""
    if kind not in _DRIFT:
        k, nx, ny, nz = PR.DARCY_SMALL[PR.DRIFT_MESH[kind]]
        om = o.build_mesh(PR.dim_of(k), k, nx, ny, nz)
        p = PR.darcy_pressures(om.coords)[0]
        _DRIFT[kind] = PR.residual_drift(k, om.cells, om.coords, p, PR.CONDUCTIVITY, o.darcy_velocity(om, p, PR.CONDUCTIVITY).T)
    return _DRIFT[kind]


def _darcy_case(gpu_ctx_factory, name, case, past):
    import torch

    kind, nx, ny, nz = case
    d = PR.dim_of(kind)
    ctx = _ctx(gpu_ctx_factory, case)
    try:
        cells, X = ctx.dofmap(), ctx.coords()
        n = ctx.n
        grid, passes = PR.darcy_launch(n)
        assert passes == (2 if past else 1)
        p = PR.darcy_pressures(X)
        u = np.stack([ctx.darcy_velocity(p[k], PR.CONDUCTIVITY).T for k in range(2)])
        for k in range(2):
            t = torch.as_tensor(p[k], device=f"cuda:{ctx.device}")
            ud = ctx.darcy_velocity_device(t, PR.CONDUCTIVITY).cpu().numpy().reshape(n, d).T
            assert np.array_equal(ud, u[k]), f"{name}: device output differs from host output (k_interleave)"
        b = PR.darcy_rhs(kind, cells, X, p, PR.CONDUCTIVITY)
        if past:
            direct = PR.kron_mass_solve((nx, ny, nz)[:d], b.reshape(2 * d, n)) if kind in (PR.QUAD, PR.HEX) else None
        else:
            om = o.build_mesh(d, kind, nx, ny, nz)
            assert np.array_equal(om.cells, cells) and np.array_equal(om.coords, X)
            direct = np.stack([o.darcy_velocity(om, p[k], PR.CONDUCTIVITY).T for k in range(2)])
        drift = _drift(kind)
        exc, fig = PR.darcy_excess(kind, cells, X, p, u, drift, direct=direct, b=b)
        print(f"{name}: {n} nodes, {grid} workgroups, {passes} pass(es) per thread ({max(n - PR.DARCY_LANES, 0)} nodes in the "
              f"second); max D / min D {fig['ratio']:.4f}, error factor {fig['factor']:.3f}, drift {drift:.2e}; "
              f"||D^-1 r|| / ||D^-1 b|| {fig['res']:.3e} (bound {fig['res_bound']:.3e}); linear pressure ||u + k a||_2 "
              f"{fig['linear']:.3e} (bound {fig['linear_bound']:.3e}); against the direct solve "
              f"{fig.get('direct', float('nan')):.3e} relative; fractions of the bounds {exc}")
        assert max(exc.values()) <= 1.0, (name, exc, fig)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(PR.DARCY_PAST))
def test_darcy_projection_past_the_launch_cap(gpu_ctx_factory, name):
    """a second node per thread in k_darcy_rhs_* and k_interleave; device output bit for bit the host output; residual of
    M u = b by the matrix-free reference; Kronecker direct solve on quadrilaterals and hexahedra; the constant for a
    linear pressure at every node, those of the second pass included"""
    _darcy_case(gpu_ctx_factory, name, PR.DARCY_PAST[name], True)


@pytest.mark.parametrize("name", list(PR.DARCY_SMALL))
def test_darcy_projection_below_the_cap_against_the_oracle(gpu_ctx_factory, name):
    """ragged meshes of a few thousand nodes, a partly filled second workgroup (quad 16 x 15), 1 and 2 cells per direction:
    against o.darcy_velocity within the derived bound, and the same residual and device-output checks"""
    _darcy_case(gpu_ctx_factory, name, PR.DARCY_SMALL[name], False)
