"""NumPy restatement of the preconditioned Lanczos iteration on the device (pph_eig_pclanczos, perphil_amd/csrc/pph_eig.hip)
and the references its tests compare against.  Not a test module: imported by test_pclanczos_host.py and
test_pclanczos_gpu.py.

The restatement follows the device code rule for rule - masked start vector, the sign scan of r.Br before the breakdown scan,
latched stopping test every `check_every` steps - but takes the extremes of T from scipy.linalg.eigh_tridiagonal instead of
the library's own host routine, so the two check each other."""
import numpy as np
from scipy.linalg import cholesky, eigh_tridiagonal

import lanczos_reference as lr

BREAKDOWN = lr.BREAKDOWN
# launch rule of k_pclanczos_update / k_pclanczos_scale: that of the plain iteration's vector kernels,
# min(ceil(ceil(n / 2) / 256), 1024) blocks of 256 threads on pairs of rows
GRID_CAPACITY_ROWS = lr.GRID_CAPACITY_ROWS
DEFAULT_TOL, DEFAULT_MAX_IT, DEFAULT_CHECK_EVERY = 1e-4, 2000, 16


def grid_blocks(n: int) -> int:
    """Blocks of the two new kernels (and of k_lanczos_dot) for n rows."""
    pairs = (n + 1) // 2
    return max(1, min((pairs + 255) // 256, 1024))


class NotPositiveDefinite(ValueError):
    """B is not positive definite on the Krylov space (the device returns PPH_ERR_INVALID: a ValueError in Python)."""


def pc_lanczos_extremes(A, apply_B, mask=None, tol: float = DEFAULT_TOL, max_it: int = DEFAULT_MAX_IT,
                        check_every: int = DEFAULT_CHECK_EVERY) -> dict:
    """Lanczos for the pencil (A, B^-1) with the device code's rules.  A: symmetric (sparse or dense) matrix with unit rows
    on the constrained dofs; apply_B(r) -> B r; mask: True on constrained rows (None: none).  Returns the fields of
    Context.preconditioned_extremes that do not depend on the device."""
    n = A.shape[0]
    mask = np.zeros(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)

    def B(r):
        z = np.array(apply_B(r), dtype=np.float64)
        z[mask] = 0.0
        return z

    u = lr.start_vector(n)
    u[mask] = 0.0
    v = B(u)
    uv = float(u @ v)
    if uv == 0.0:
        raise ValueError("no free rows")
    if not (uv > 0.0 and np.isfinite(uv)):
        raise NotPositiveDefinite(f"start: u.Bu = {uv:.3e}")
    b = np.sqrt(uv)
    u, v = u / b, v / b
    uprev = np.zeros(n)
    alpha, beta, rz = np.zeros(max_it), np.zeros(max_it), np.zeros(max_it)
    conv = [False, False]
    m = 0
    with np.errstate(all="ignore"):
        while True:
            m1 = min(m + check_every, max_it)
            for j in range(m, m1):
                w = A @ v
                alpha[j] = v @ w
                r = w - alpha[j] * u - (beta[j - 1] * uprev if j > 0 else 0.0)
                z = B(r)
                rz[j] = r @ z
                beta[j] = np.sqrt(rz[j])
                inv = 1.0 / beta[j]
                uprev, u, v = u, r * inv, z * inv
            m = m1
            scale = beta[0] if np.isfinite(beta[0]) else 0.0
            for j in range(m):
                scale = max(scale, abs(alpha[j]))
                if rz[j] < -BREAKDOWN * scale * scale:
                    raise NotPositiveDefinite(f"step {j}: r.Br = {rz[j]:.3e}")
                if not np.isfinite(beta[j]) or not beta[j] > BREAKDOWN * scale:
                    lo, hi, _, _ = lr._extremes(alpha, beta, j + 1)
                    return {"lambda_min": lo, "lambda_max": hi, "iterations": m, "converged": 1, "breakdown": 1,
                            "krylov_dimension": j + 1, "estimate_min": 0.0, "estimate_max": 0.0, "kappa": hi / lo}
            lo, hi, sl, sh = lr._extremes(alpha, beta, m)
            est = [abs(beta[m - 1] * sl), abs(beta[m - 1] * sh)]
            for e, th in enumerate((lo, hi)):
                if est[e] <= tol * abs(th):
                    conv[e] = True
            if all(conv) or m >= max_it:
                return {"lambda_min": lo, "lambda_max": hi, "iterations": m, "converged": int(all(conv)), "breakdown": 0,
                        "krylov_dimension": m, "estimate_min": est[0], "estimate_max": est[1], "kappa": hi / lo}


# ---- dense references -------------------------------------------------------------------------------------------------
def dense_operator(apply_B, n: int, free: np.ndarray) -> np.ndarray:
    """B on the free rows, column by column: B_ff[:, k] = (B e_free[k])[free]."""
    Bf = np.zeros((len(free), len(free)))
    e = np.zeros(n)
    for k, i in enumerate(free):
        e[i] = 1.0
        Bf[:, k] = np.asarray(apply_B(e))[free]
        e[i] = 0.0
    return Bf


def dense_pencil(A, Bff: np.ndarray, free: np.ndarray) -> dict:
    """Eigenvalues of C^T sym(B_ff) C with A_ff = C C^T (the spectrum of B A on the free rows), and a = ||E||_2 ||A_ff||_2
    with E the skew part of B_ff: the distance, in eigenvalue units, between B and the symmetric operator the reference
    takes (a perturbation E of B moves the eigenvalues of C^T B C by at most ||C||_2^2 ||E||_2)."""
    Aff = (A[free][:, free]).toarray() if hasattr(A, "toarray") else np.asarray(A)[np.ix_(free, free)]
    C = cholesky(Aff, lower=True)
    S, E = 0.5 * (Bff + Bff.T), 0.5 * (Bff - Bff.T)
    ev = np.linalg.eigvalsh(C.T @ S @ C)
    a = np.linalg.norm(E, 2) * np.linalg.norm(Aff, 2)
    return {"lambda_min": float(ev[0]), "lambda_max": float(ev[-1]), "a": float(a), "eigenvalues": ev}


# ---- closed form: the Jacobi-scaled mass matrix on a box ---------------------------------------------------------------
def box_scaled_mass_extremes(cells):
    """(lambda_min, lambda_max) of D^-1 M, M the multilinear mass matrix on the unit box of `cells` cells without Dirichlet
    rows: M is the Kronecker product of the 1D mass matrices and the diagonal of a Kronecker product is the Kronecker product
    of the diagonals, so the pencil (M, diag M) factors and its extremes are the products of those of the 1D pencils
    (M_1, diag M_1) - which are 1/2 and 3/2 for every cell count (eigenvectors (-1)^i and 1): hexes give (1/8, 27/8)."""
    lo = hi = 1.0
    for N in cells:
        M1 = lr.mass_1d(N)
        s = 1.0 / np.sqrt(np.diag(M1))
        S = M1 * s[:, None] * s[None, :]   # tridiagonal
        ev = eigh_tridiagonal(np.diag(S), np.diag(S, 1), eigvals_only=True)
        lo, hi = lo * ev[0], hi * ev[-1]
    return float(lo), float(hi)
