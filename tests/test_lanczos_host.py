"""CPU checks behind the device Lanczos path (pph_eig.hip): the NumPy restatement of the iteration
(lanczos_reference.py) reproduces the reference's conditioning goldens G3, G4 and G5 on the oracle's matrices - every row,
the ones dense algebra is too slow for included -, the library's host routine for the extremes of the tridiagonal matrix
(pph_tridiag_extremes: Sturm bisection + inverse iteration, no device touched) against closed forms and
scipy.linalg.eigh_tridiagonal, and the closed-form spectra test_lanczos_gpu.py uses against dense eigenvalues."""
import numpy as np
import pytest
from scipy.linalg import eigh_tridiagonal

import lanczos_reference as lr
from oracle import dpp_oracle as o

P = o.Params(k1=1.0, k2=0.01, beta=1.0, mu=1.0)


def _kappas(s):
    n = s.n
    A = s.A.tocsr()
    out = []
    for B in (A, A[:n, :n].tocsr(), A[n:, n:].tocsr()):
        r = lr.lanczos_extremes(B)
        assert r["converged"] == 1
        out.append(r["lambda_max"] / r["lambda_min"])
    return out


def test_restatement_reproduces_G3(goldens):
    g = goldens["G3_condition_numbers_10x10"]
    k = _kappas(o.build_system(o.build_mesh(2, o.CELL_QUAD, 10, 10), P))
    assert k == pytest.approx([g["monolithic"], g["macro"], g["micro"]], rel=1e-10)


@pytest.mark.parametrize("row", [0, 1, 2, 3, 4])
def test_restatement_reproduces_G4(goldens, row):
    """conditioning.csv, all five rows (N = 4 .. 64; homogeneous data, DPPParameters())."""
    g = goldens["G4_conditioning_2d"][row]
    N = int(g["N"])
    k = _kappas(o.build_system(o.build_mesh(2, o.CELL_QUAD, N, N), o.Params(), mms=False))
    assert k == pytest.approx([g["cond_monolithic"], g["cond_macro"], g["cond_micro"]], rel=1e-10)


@pytest.mark.parametrize("row", [0, 1, 2, 3, 4, 5, 6])
def test_restatement_reproduces_G5(goldens, row):
    """conditioning_3d.csv, all seven rows (N = 4 .. 16)."""
    g = goldens["G5_conditioning_3d_hex"][row]
    N = int(g["N"])
    s = o.build_system(o.build_mesh(3, o.CELL_HEX, N, N, N), P)
    assert 2 * s.n == int(g["n_dofs"])
    assert _kappas(s) == pytest.approx([g["cond_monolithic"], g["cond_macro"], g["cond_micro"]], rel=1e-10)


def test_restatement_breaks_down_on_tiny_boxes():
    """N = 1: the operator is the identity, one step; N = 2: one interior node per field - two distinct eigenvalues in a
    block, three in the monolithic system.  The truncated T gives them exactly (to rounding)."""
    for dim, kind in ((2, o.CELL_QUAD), (2, o.CELL_TRI), (3, o.CELL_HEX), (3, o.CELL_TET)):
        for N, dims in ((1, (1, 1, 1)), (2, (3, 2, 2))):
            s = o.build_system(o.build_mesh(dim, kind, N, N, N if dim == 3 else 0), P, mms=False)
            n = s.n
            A = s.A.tocsr()
            for B, want in ((A, dims[0]), (A[:n, :n], dims[1]), (A[n:, n:], dims[2])):
                r = lr.lanczos_extremes(B.tocsr())
                ev = np.linalg.eigvalsh(B.toarray())
                assert r["breakdown"] == 1 and r["iterations"] == 32 and r["krylov_dimension"] == want
                assert r["lambda_min"] == pytest.approx(ev[0], rel=1e-12) and r["lambda_max"] == pytest.approx(ev[-1], rel=1e-12)


# ---- pph_tridiag_extremes through ctypes (fails without the feature: the symbol does not exist) -----------------------
def _check_tridiag(alpha, beta, want):
    from perphil_amd import _ffi

    got = _ffi.tridiag_extremes(alpha, beta)
    bar = 1e-14 * max(abs(want[0]), abs(want[1]))
    assert abs(got[0] - want[0]) <= bar and abs(got[1] - want[1]) <= bar, (got, want)
    assert abs(abs(got[2]) - abs(want[2])) <= 1e-9 and abs(abs(got[3]) - abs(want[3])) <= 1e-9, (got, want)


@pytest.mark.parametrize("m", [1, 2, 3, 64, 1000])
def test_tridiag_extremes_of_the_1d_laplacian(m):
    _check_tridiag(np.full(m, 2.0), np.full(m - 1, -1.0), lr.laplacian_tridiag_extremes(m))


@pytest.mark.parametrize("m,seed", [(2, 0), (5, 1), (17, 2), (100, 3), (333, 4)])
def test_tridiag_extremes_of_random_matrices(m, seed):
    rng = np.random.default_rng(seed)
    alpha, beta = rng.uniform(-1.0, 3.0, m), rng.uniform(0.2, 1.5, m - 1)
    w, z = eigh_tridiagonal(alpha, beta)
    _check_tridiag(alpha, beta, (w[0], w[-1], z[-1, 0], z[-1, -1]))


def test_tridiag_extremes_of_a_lanczos_matrix():
    """The matrix the device would hand over: T of 96 plain Lanczos steps on the hex 6^3 monolithic system (ends converging,
    entries spread over four decades)."""
    A = o.build_system(o.build_mesh(3, o.CELL_HEX, 6, 6, 6), P).A.tocsr()
    v, vprev, alpha, beta = lr.start_vector(A.shape[0]), 0.0, [], []
    for j in range(96):
        w = A @ v
        alpha.append(v @ w)
        r = w - alpha[-1] * v - (beta[-1] * vprev if j else 0.0)
        beta.append(np.linalg.norm(r))
        vprev, v = v, r / beta[-1]
    alpha, beta = np.array(alpha), np.array(beta[:-1])
    w, z = eigh_tridiagonal(alpha, beta)
    _check_tridiag(alpha, beta, (w[0], w[-1], z[-1, 0], z[-1, -1]))


@pytest.mark.parametrize("scale", [2.0 ** -900, 2.0 ** 900])
def test_tridiag_extremes_in_any_units(scale):
    """Entries whose squares leave the exponent range: the routine works on T scaled by a power of two (exact)."""
    m = 64
    lo, hi, sl, sh = lr.laplacian_tridiag_extremes(m)
    _check_tridiag(np.full(m, 2.0) * scale, np.full(m - 1, -1.0) * scale, (lo * scale, hi * scale, sl, sh))


def test_tridiag_extremes_refuses_bad_arguments():
    from perphil_amd import _ffi

    with pytest.raises(ValueError):
        _ffi.tridiag_extremes(np.zeros(0), np.zeros(0))
    with pytest.raises(ValueError):
        _ffi.tridiag_extremes(np.array([1.0, np.nan]), np.array([0.5]))


# ---- closed forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,kind,cells", [(2, o.CELL_QUAD, (12, 9)), (3, o.CELL_HEX, (5, 4, 3))])
def test_closed_forms_match_dense_eigenvalues(dim, kind, cells):
    Pc = o.Params(k1=1.0, k2=0.01, beta=3.0, mu=2.0)
    m = o.build_mesh(dim, kind, *cells)
    s = o.build_system(m, Pc, mms=False)
    n = s.n
    a, b, c = Pc.abc
    for B, ck in ((s.A[:n, :n], a), (s.A[n:, n:], c)):
        ev = np.linalg.eigvalsh(B.toarray())
        assert lr.box_block_extremes(cells, ck, b) == pytest.approx((ev[0], ev[-1]), rel=1e-13)
    _, M = o.assemble_scalar(m)
    ev = np.linalg.eigvalsh(M.toarray())
    assert lr.box_mass_extremes(cells) == pytest.approx((ev[0], ev[-1]), rel=1e-13)


def test_start_vector_is_the_product_benchmarks_hash():
    """k_fill_pattern's hash (pph_api.hip) restated with Python integers."""
    raw = []
    for i in range(7):
        h = (i * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & (2**64 - 1)
        h ^= h >> 29
        h = (h * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        h ^= h >> 32
        raw.append((h >> 11) * (2.0 / 9007199254740992.0) - 1.0)
    raw = np.array(raw)
    assert np.all(np.abs(raw) < 1.0) and len(set(raw)) == 7
    np.testing.assert_allclose(lr.start_vector(7), raw / np.linalg.norm(raw), rtol=1e-15)
