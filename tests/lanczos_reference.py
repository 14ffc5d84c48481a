"""NumPy restatement of the device Lanczos iteration (perphil_amd/csrc/pph_eig.hip) and the closed-form spectra its
tests compare against.  Not a test module: imported by test_lanczos_host.py and test_lanczos_gpu.py.

The restatement follows the device code rule for rule - start vector, breakdown scan, latched stopping test every
`check_every` steps - but takes the extremes of T from scipy.linalg.eigh_tridiagonal instead of the library's own host
routine, so the two check each other."""
import numpy as np
from scipy.linalg import eigh_tridiagonal

BREAKDOWN = 1e-13
# launch rule of k_lanczos_update / k_lanczos_scale: min(ceil(ceil(n / 2) / 256), 1024) blocks of 256 threads, two rows per
# thread and pass - a thread takes a second pair of rows when n exceeds this
GRID_CAPACITY_ROWS = 1024 * 256 * 2


def start_vector(n: int) -> np.ndarray:
    """The hash of k_fill_pattern (pph_api.hip) over the row index, in (-1, 1), normalised."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    v = (h >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0
    return v / np.linalg.norm(v)


def _extremes(alpha, beta, m):
    """theta_min, theta_max and the last components of their eigenvectors of T's leading m rows."""
    if m == 1:
        return alpha[0], alpha[0], 1.0, 1.0
    lo, zl = eigh_tridiagonal(alpha[:m], beta[:m - 1], select="i", select_range=(0, 0))
    hi, zh = eigh_tridiagonal(alpha[:m], beta[:m - 1], select="i", select_range=(m - 1, m - 1))
    return float(lo[0]), float(hi[0]), float(zl[-1, 0]), float(zh[-1, 0])


def lanczos_extremes(A, tol: float = 1e-10, max_it: int = 20000, check_every: int = 32) -> dict:
    """Plain symmetric Lanczos on the (sparse or dense) symmetric matrix A with the device code's rules.  Returns the
    fields of Context.extreme_eigenvalues that do not depend on the device."""
    n = A.shape[0]
    v = start_vector(n)
    vprev = np.zeros(n)
    alpha, beta = np.zeros(max_it), np.zeros(max_it)
    conv = [False, False]
    m = 0
    with np.errstate(all="ignore"):
        while True:
            m1 = min(m + check_every, max_it)
            for j in range(m, m1):
                w = A @ v
                alpha[j] = v @ w
                r = w - alpha[j] * v - (beta[j - 1] * vprev if j > 0 else 0.0)
                beta[j] = np.sqrt(r @ r)
                vprev, v = v, r * (1.0 / beta[j])
            m = m1
            scale = beta[0] if np.isfinite(beta[0]) else 0.0
            for j in range(m):
                scale = max(scale, abs(alpha[j]))
                if not np.isfinite(beta[j]) or not beta[j] > BREAKDOWN * scale:
                    lo, hi, _, _ = _extremes(alpha, beta, j + 1)
                    return {"lambda_min": lo, "lambda_max": hi, "iterations": m, "converged": 1, "breakdown": 1,
                            "krylov_dimension": j + 1, "estimate_min": 0.0, "estimate_max": 0.0}
            lo, hi, sl, sh = _extremes(alpha, beta, m)
            est = [abs(beta[m - 1] * sl), abs(beta[m - 1] * sh)]
            for e, th in enumerate((lo, hi)):
                if est[e] <= tol * abs(th):
                    conv[e] = True
            if all(conv) or m >= max_it:
                return {"lambda_min": lo, "lambda_max": hi, "iterations": m, "converged": int(all(conv)), "breakdown": 0,
                        "krylov_dimension": m, "estimate_min": est[0], "estimate_max": est[1]}


# ---- closed forms ---------------------------------------------------------------------------------------------------
def laplacian_tridiag_extremes(m: int):
    """T = tridiag(-1, 2, -1) of m rows: (theta_min, theta_max, |last component| of either normalised eigenvector)."""
    th = lambda k: 2.0 - 2.0 * np.cos(k * np.pi / (m + 1))
    last = lambda k: abs(np.sqrt(2.0 / (m + 1)) * np.sin(m * k * np.pi / (m + 1)))
    return th(1), th(m), last(1), last(m)


def _modes_1d(N: int):
    """Eigenvalues of the 1D P1 stiffness and mass matrices of N cells on [0, 1] without their end nodes (one set of
    eigenvectors: sin(k pi x))."""
    h = 1.0 / N
    c = np.cos(np.arange(1, N) * np.pi / N)
    return (2.0 - 2.0 * c) / h, h * (4.0 + 2.0 * c) / 6.0


def box_block_extremes(cells, coef_K: float, coef_M: float):
    """(lambda_min, lambda_max) of coef_K K + coef_M M of multilinear elements (quads, hexes) on the unit box of `cells` =
    (nx, ny[, nz]) cells with Dirichlet rows (unit diagonal) on the whole boundary:
    {1} U {coef_K sum_d kappa_d prod_{e != d} mu_e + coef_M prod_d mu_d}."""
    modes = [_modes_1d(N) for N in cells]
    d = len(modes)
    shape = lambda a, ax: a.reshape([-1 if i == ax else 1 for i in range(d)])
    mass = 1.0
    for ax in range(d):
        mass = mass * shape(modes[ax][1], ax)
    lam = coef_M * mass
    for ax in range(d):
        t = shape(modes[ax][0], ax)
        for o in range(d):
            if o != ax:
                t = t * shape(modes[o][1], o)
        lam = lam + coef_K * t
    lam = np.append(lam.ravel(), 1.0)
    return float(lam.min()), float(lam.max())


def mass_1d(N: int) -> np.ndarray:
    """Dense 1D P1 mass matrix of N cells on [0, 1], all N + 1 nodes."""
    h = 1.0 / N
    M = np.zeros((N + 1, N + 1))
    i = np.arange(N + 1)
    M[i, i] = 4.0 * h / 6.0
    M[0, 0] = M[N, N] = 2.0 * h / 6.0
    M[i[:-1], i[1:]] = M[i[1:], i[:-1]] = h / 6.0
    return M


def box_mass_extremes(cells):
    """(lambda_min, lambda_max) of the multilinear mass matrix on the unit box without Dirichlet rows: the Kronecker
    product of the 1D mass matrices, so the products of their (positive) extremes."""
    lo = hi = 1.0
    for N in cells:
        ev = np.linalg.eigvalsh(mass_1d(N))
        lo, hi = lo * ev[0], hi * ev[-1]
    return float(lo), float(hi)
