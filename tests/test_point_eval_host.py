"""Point evaluation without a GPU: the longdouble restatement checks itself (partition of unity, polynomial reproduction,
nodal values, brute force against the vectorised variant), the Python layer refuses bad input before any context exists,
and the share of random points the GPU gradient test leaves out is within its cap."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import point_eval_reference as PR  # noqa: E402

LD = np.longdouble
KD = [(c, deg) for c in PR.CASES for deg in (1, 2)]
IDS = [f"{('quad', 'tri', 'hex', 'tet')[c[0]]}-deg{deg}" for c, deg in KD]
EPS_LD = float(np.finfo(LD).eps)


def _points(kind, nx, ny, nz, count=150):
    return np.concatenate([PR.random_points(kind, 1, count), PR.deliberate_points(kind, nx, ny, nz)[::7]])


@pytest.mark.parametrize("case,deg", KD, ids=IDS)
def test_partition_of_unity(case, deg):
    kind, nx, ny, nz = case
    X = _points(kind, nx, ny, nz)
    ones = np.ones(PR.n_nodes(kind, deg, nx, ny, nz))
    for r in (PR.evaluate(kind, deg, nx, ny, nz, ones, X), PR.evaluate_fast(kind, deg, nx, ny, nz, ones, X)):
        assert np.abs(r["v"] - 1).max() <= 64 * EPS_LD
        assert np.abs(r["g"]).max() <= 64 * EPS_LD * max(nx, ny, nz) * 30


@pytest.mark.parametrize("case,deg", KD, ids=IDS)
def test_reproduces_the_polynomials_of_the_space(case, deg):
    kind, nx, ny, nz = case
    d = PR.dim_of(kind)
    f = PR.integer_polynomial(kind, deg, nx, ny, nz)
    ids = np.arange(PR.n_nodes(kind, deg, nx, ny, nz))
    u = f(PR.lattice_index(ids, kind, deg, nx, ny, nz).astype(np.float64))
    X = PR.random_points(kind, deg, 200)
    T = X.astype(LD) * (deg * PR.boxes(kind, nx, ny, nz)).astype(LD)
    exact = f(T)
    h = LD(1e-6)
    for r in (PR.evaluate(kind, deg, nx, ny, nz, u, X), PR.evaluate_fast(kind, deg, nx, ny, nz, u, X)):
        assert np.abs(r["v"][:, 0] - exact).max() <= 256 * EPS_LD * np.abs(u).max()
        for e in range(d):      # gradient against a central difference of the polynomial (exact for quadratics up to rounding)
            Tp, Tm = T.copy(), T.copy()
            Tp[:, e] += h; Tm[:, e] -= h
            dfdx = (f(Tp) - f(Tm)) / (2 * h) * (deg * PR.boxes(kind, nx, ny, nz)[e])
            far = PR.face_distance(kind, nx, ny, nz, X) > 1e-5
            assert np.abs(r["g"][far, 0, e] - dfdx[far]).max() <= 1e-9 * np.abs(dfdx).max()


@pytest.mark.parametrize("case,deg", KD, ids=IDS)
def test_value_at_a_node_is_the_coefficient(case, deg):
    kind, nx, ny, nz = case
    u = PR.random_coefficients(kind, deg, nx, ny, nz)
    ids = np.arange(0, len(u), 3)
    X = PR.node_coords(ids, kind, deg, nx, ny, nz).astype(np.float64)
    r = PR.evaluate(kind, deg, nx, ny, nz, u, X)
    # the double coordinates of a node are rounded: the node is met to within the bound's own xi term
    assert np.all(np.abs(r["v"] - u[ids]) <= PR.value_bound(kind, deg, nx, ny, nz, r))


@pytest.mark.parametrize("case,deg", KD, ids=IDS)
def test_brute_force_and_vectorised_variants_agree(case, deg):
    kind, nx, ny, nz = case
    u = PR.random_coefficients(kind, deg, nx, ny, nz, ncomp=2)
    X = PR.random_points(kind, deg, 300)
    a = PR.evaluate(kind, deg, nx, ny, nz, u, X)
    b = PR.evaluate_fast(kind, deg, nx, ny, nz, u, X)
    for key in ("v", "g", "S", "G", "H"):
        scale = np.abs(a[key]).max()
        assert np.abs(a[key] - b[key]).max() <= 1e3 * EPS_LD * scale, key
    # sub-cell chosen by the fast variant = position of the brute-force cell in its box
    cpb = {PR.QUAD: 1, PR.TRI: 2, PR.HEX: 1, PR.TET: 6}[kind]
    assert np.array_equal(a["cell"] % cpb, b["sub"])


def test_outside_and_clamped_points_in_the_restatement():
    kind, nx, ny, nz = PR.CASES[0]
    u = PR.random_coefficients(kind, 1, nx, ny, nz)
    X = np.array([[0.5, 0.5], [1.0 + 1e-13 / nx, 0.5], [1.0 + 1e-11, 0.5], [0.5, -1e-3], [np.nan, 0.2]])
    for r in (PR.evaluate(kind, 1, nx, ny, nz, u, X), PR.evaluate_fast(kind, 1, nx, ny, nz, u, X)):
        assert list(r["outside"]) == [False, False, True, True, True]
        assert list(np.isnan(r["v"][:, 0])) == [False, False, True, True, True]


@pytest.mark.parametrize("case,deg", KD, ids=IDS)
def test_share_of_points_the_gradient_test_leaves_out(case, deg):
    """The GPU gradient test drops random points closer than 1e-6 box-local units to a cell or sub-cell face; with uniform
    points the expected share is about 1e-5, the cap is 1 %."""
    kind, nx, ny, nz = case
    X = PR.random_points(kind, deg)
    left_out = np.count_nonzero(PR.face_distance(kind, nx, ny, nz, X) <= 1e-6)
    assert left_out <= 0.01 * len(X)


# ------------------------------------------------------------------------------------------------------------------
# Python-side refusals: nothing here may create a device context
# ------------------------------------------------------------------------------------------------------------------
def _no_context(mesh):
    return mesh._ctx is None and not mesh.__dict__.get("_ctx_deg")


@pytest.mark.parametrize("deg", (1, 2))
@pytest.mark.parametrize("dim", (2, 3))
def test_refusals_create_no_context(dim, deg):
    from perphil_amd import fd

    mesh = fd.UnitSquareMesh(4, 3, quadrilateral=True) if dim == 2 else fd.UnitCubeMesh(3, 2, 2)
    V = fd.FunctionSpace(mesh, "CG", deg)
    f = fd.Function(V).interpolate(lambda X: X[:, 0] + 2 * X[:, 1])
    inside = [0.3] * dim
    for bad in ([0.3] * (dim + 1), [[0.3] * (dim + 1)], np.zeros((2, 2, dim)), 0.5):
        with pytest.raises(ValueError):
            f.at(bad)
        with pytest.raises(ValueError):
            f.gradient_at(bad)
    with pytest.raises(ValueError):
        f.at(inside, tolerance=0.7)
    far = [1.5] + [0.5] * (dim - 1)
    with pytest.raises(fd.PointNotInDomainError) as e:
        f.at([inside, far, [-2.0] * dim])
    assert "1.5" in str(e.value) and "index 1" in str(e.value)
    with pytest.raises(fd.PointNotInDomainError):
        f.at(far)
    with pytest.raises(fd.PointNotInDomainError):
        f.gradient_at([far])
    with pytest.raises(fd.PointNotInDomainError):      # outside by more than the default tolerance, in box-local units
        f.at([1.0 + 1e-11, 0.37] + [0.5] * (dim - 2))
    v = f.at([far, [-2.0] * dim], dont_raise=True)
    assert v.shape == (2,) and np.isnan(v).all()
    g = f.gradient_at([far], dont_raise=True)
    assert g.shape == (1, dim) and np.isnan(g).all()
    assert np.isnan(f.at(far, dont_raise=True))
    assert _no_context(mesh)


def test_refusals_on_mixed_and_vector_functions_create_no_context():
    from perphil_amd import fd

    mesh = fd.UnitSquareMesh(4, 3)
    V = fd.FunctionSpace(mesh, "CG", 1)
    w = fd.Function(V * V)
    r = w.at([[2.0, 0.5]], dont_raise=True)
    assert isinstance(r, tuple) and len(r) == 2 and all(np.isnan(x).all() and x.shape == (1,) for x in r)
    u = fd.Function(fd.VectorFunctionSpace(mesh, "CG", 1))
    assert u.at([[2.0, 0.5], [0.5, 3.0]], dont_raise=True).shape == (2, 2)
    assert u.gradient_at([[2.0, 0.5]], dont_raise=True).shape == (1, 2, 2)
    with pytest.raises(fd.PointNotInDomainError):
        w.at((0.5, 1.25))
    assert _no_context(mesh)


def test_a_node_of_the_space_keeps_the_coefficient_without_a_context():
    from perphil_amd import fd

    mesh = fd.UnitSquareMesh(4, 3)
    for deg in (1, 2):
        V = fd.FunctionSpace(mesh, "CG", deg)
        vals = np.random.default_rng(deg).standard_normal(V.dim())
        f = fd.Function(V, vals.copy())
        X = mesh.node_coordinates(degree=deg)
        for k in (0, 5, V.dim() - 1):
            assert f.at(tuple(X[k])) == vals[k]
            assert f.at(X[k] + 4e-10 / (deg * 4)) == vals[k]      # today's 1e-9 snapping rule
    assert _no_context(mesh)
