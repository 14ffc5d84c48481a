"""
Matrix export + condition numbers — mirror of reference ``src/perphil/solvers/conditioning.py``
(SURVEY.md §8f rank 4): ``get_matrix_data_from_form`` (:66-102) assembles on the device and returns the
SciPy CSR the reference extracts from PETSc (``getValuesCSR`` + ``eliminate_zeros``);
``calculate_condition_number`` (:105-218) is the same dense-SVD / extreme-singular-value computation the
reference runs in SciPy on the host (it is analysis code there as well, not part of the solve).
"""
from __future__ import annotations

from typing import List, Optional

import attr
import numpy as np
from scipy.sparse import csr_matrix

from . import _ffi, fd
from .forms import DPPBilinearForm, ScalarBlockForm

DEFAULT_CONDITION_NUMBER_TOLERANCE = 1e-7


@attr.define(frozen=True)
class MatrixData:
    """Same fields as the reference's MatrixData minus the PETSc handles (there is no PETSc here)."""
    is_symmetric: bool
    sparse_csr_data: csr_matrix
    number_of_nonzero_entries: int
    number_of_dofs: int
    symmetry_tolerance: float


def _set_bcs(ctx, space, bcs: List[fd.DirichletBC]) -> None:
    empty = (np.zeros(0, np.int64), np.zeros(0))
    per_field = {0: empty, 1: empty}
    for bc in bcs or []:
        per_field[bc.field] = bc.nodes_and_values()
    for f in (0, 1):
        ctx.set_dirichlet(f, *per_field[f])


def _context(space):
    """The mesh's context for the degree of `space` (mixed: of its first sub space)."""
    V = space.sub(0) if isinstance(space, fd.MixedFunctionSpace) else space
    deg = getattr(V, "degree", 1)
    return space.mesh().context() if deg == 1 else space.mesh().context(degree=deg)


def get_matrix_data_from_form(form, boundary_conditions: List[fd.DirichletBC], symmetry_tolerance: float = 1e-8) -> MatrixData:
    """Assemble `form` (monolithic DPP form or one Picard block) with the BCs and export it as SciPy CSR."""
    ctx, which = _assemble_for(form, boundary_conditions)
    csr = ctx.csr(which)
    csr = csr_matrix(csr)
    csr.eliminate_zeros()
    asym = abs(csr - csr.T)
    is_symmetric = bool((asym.max() if asym.nnz else 0.0) <= symmetry_tolerance)
    return MatrixData(is_symmetric, csr, int(csr.nnz), int(csr.shape[0]), symmetry_tolerance)


def _assemble_for(form, boundary_conditions: List[fd.DirichletBC]):
    """Assembles `form` on its mesh's context as get_matrix_data_from_form does; returns (context, matrix selector)."""
    if form.space.mesh().distributed:
        raise NotImplementedError("matrix export is an analysis path on the whole matrix: build the mesh with "
                                  "comm=fd.COMM_SELF under torch.distributed")
    if isinstance(form, DPPBilinearForm):
        ctx = _context(form.space)
        _set_bcs(ctx, form.space, boundary_conditions)
        ctx.assemble(form.k1, form.k2, form.beta, form.mu, monolithic=True)
        return ctx, _ffi.MAT_MONO
    if isinstance(form, ScalarBlockForm) and form.rank == 2:
        ctx = _context(form.space)
        # a scalar block (coef_K K + coef_M M): assemble the pair with the block's coefficients on its own field
        bcs = [fd.DirichletBC(_as_field(bc, form.field), bc.value, bc.sub_domain) for bc in boundary_conditions or []]
        _set_bcs(ctx, form.space, bcs)
        k = form.coef_K if form.coef_K > 0 else 1.0
        ctx.assemble(k, k, form.coef_M, 1.0, monolithic=False)
        return ctx, (_ffi.MAT_A11 if form.field == 0 else _ffi.MAT_A22)
    raise TypeError(f"cannot assemble {type(form)}")


def _kappa_on_device(ctx, which: int, tol: float, zero_tol: float) -> float:
    r = ctx.extreme_eigenvalues(which, tol=tol)
    if not r["converged"]:
        raise RuntimeError(f"Lanczos did not converge in {r['iterations']} steps: lambda_min {r['lambda_min']:.6e} "
                           f"(estimate {r['estimate_min']:.1e}), lambda_max {r['lambda_max']:.6e} (estimate {r['estimate_max']:.1e})")
    if r["lambda_min"] <= zero_tol:
        return float("inf")
    return float(r["lambda_max"] / r["lambda_min"])


def condition_number_on_device(form, boundary_conditions: List[fd.DirichletBC], tol: float = 1e-10,
                               zero_tol: float = DEFAULT_CONDITION_NUMBER_TOLERANCE) -> float:
    """kappa = lambda_max / lambda_min of the assembled `form` (the forms get_matrix_data_from_form accepts: symmetric
    positive definite after the symmetric Dirichlet elimination, so singular values are eigenvalues) by Lanczos on the
    device: assembled like get_matrix_data_from_form, nothing exported.  inf when lambda_min does not exceed `zero_tol`
    (the reference's sparse branch, conditioning.py:204-209); RuntimeError when the iteration did not converge."""
    ctx, which = _assemble_for(form, boundary_conditions)
    return _kappa_on_device(ctx, which, tol, zero_tol)


_PC_NAMES = {"jacobi": _ffi.PC_JACOBI, "pph_block2": _ffi.PC_BLOCK2, "ilu": _ffi.PC_ILU, "mg": _ffi.PC_MG, "pph_pmg": _ffi.PC_PMG,
             "pph_cmg": _ffi.PC_CMG}
_BLOCK_PCS = ("jacobi", "ilu", "mg", "pph_pmg")
_MONOLITHIC_PCS = ("jacobi", "pph_block2", "ilu", "pph_cmg")


def _space_degree(space) -> int:
    V = space.sub(0) if isinstance(space, fd.MixedFunctionSpace) else space
    return int(getattr(V, "degree", 1))


def _check_preconditioned_pairing(monolithic: bool, space, pc_type: str) -> None:
    """NotImplementedError for every (operator, pc_type) pairing pph_preconditioned_extremes refuses - raised before any
    context exists, so a refusal never touches a GPU."""
    if space.mesh().distributed:
        raise NotImplementedError("preconditioned condition numbers work on the whole operator on one device: build the mesh "
                                  "with comm=fd.COMM_SELF under torch.distributed")
    if pc_type == "none":
        raise NotImplementedError("pc_type 'none' is the operator itself: use condition_number_on_device")
    if pc_type == "fieldsplit":
        raise NotImplementedError("the multiplicative field split is not a symmetric preconditioner: B A has no Lanczos "
                                  "recurrence; ask for its blocks (effective_condition_numbers)")
    if pc_type not in _PC_NAMES:
        raise NotImplementedError(f"pc_type {pc_type!r} is not supported ({', '.join(_PC_NAMES)})")
    allowed = _MONOLITHIC_PCS if monolithic else _BLOCK_PCS
    if pc_type not in allowed:
        what = "the monolithic system" if monolithic else "a scalar block"
        raise NotImplementedError(f"pc_type {pc_type!r} does not precondition {what} (there: {', '.join(allowed)})")
    if pc_type == "mg" and _space_degree(space) != 1:
        raise NotImplementedError("degree-2 spaces have no CG-1-only multigrid hierarchy: pc_type 'mg' is not available; "
                                  "use 'pph_pmg'")
    if pc_type == "pph_cmg" and _space_degree(space) != 1:
        raise NotImplementedError("pc_type 'pph_cmg' is a cycle on the CG-1 multigrid hierarchy: degree-2 spaces have none")


def _pc_kappa(ctx, which: int, pc_type: str, mg_smooth: int, tol: float) -> float:
    r = ctx.preconditioned_extremes(which, _PC_NAMES[pc_type], mg_smooth=mg_smooth, tol=tol)
    if not r["converged"]:
        raise RuntimeError(f"preconditioned Lanczos ({pc_type}) did not converge in {r['iterations']} steps: lambda_min "
                           f"{r['lambda_min']:.6e} (estimate {r['estimate_min']:.1e}), lambda_max {r['lambda_max']:.6e} "
                           f"(estimate {r['estimate_max']:.1e})")
    return float(r["kappa"])


def preconditioned_condition_number(form, boundary_conditions: List[fd.DirichletBC], pc_type: str, mg_smooth: int = 2,
                                    tol: float = 1e-4) -> float:
    """kappa(B A) = lambda_max / lambda_min of the assembled `form` (the forms get_matrix_data_from_form accepts) under the
    preconditioner `pc_type` - "jacobi", "pph_block2", "ilu", "mg", "pph_pmg" or "pph_cmg", the strings translate_options knows - on
    the FREE rows: what a Krylov method under that preconditioner sees.  Lanczos in the B inner product on the device
    (pph_preconditioned_extremes): assembled like get_matrix_data_from_form, nothing exported.  A scalar block takes jacobi,
    ilu, mg (degree 1) and pph_pmg; the monolithic form jacobi, pph_block2, ilu and pph_cmg (degree 1).  NotImplementedError, before any context
    exists, for every other pairing, for "fieldsplit" (not symmetric), "none" (condition_number_on_device) and distributed
    meshes; RuntimeError when the iteration did not converge.  The default tol 1e-4 is four digits of kappa: under multigrid
    the Ritz residual of the clustered upper end shrinks far more slowly than its value moves."""
    if not isinstance(form, DPPBilinearForm) and not (isinstance(form, ScalarBlockForm) and form.rank == 2):
        raise TypeError(f"cannot assemble {type(form)}")
    _check_preconditioned_pairing(isinstance(form, DPPBilinearForm), form.space, pc_type)
    ctx, which = _assemble_for(form, boundary_conditions)
    return _pc_kappa(ctx, which, pc_type, mg_smooth, tol)


def effective_condition_numbers(W, params, bcs: List[fd.DirichletBC], solver_parameters: dict, nonlinear: bool = False,
                                tol: float = 1e-4) -> dict:
    """The condition numbers the Krylov methods of one option set work against: `solver_parameters` goes through
    solver.translate_options, and what that configuration preconditions is measured with preconditioned_condition_number's
    rules.  A monolithic pc_type (jacobi, pph_block2, ilu, pph_cmg) gives {"monolithic": kappa(B A)}; a field split or Picard sweeps
    give {"macro": kappa(B1 A11), "micro": kappa(B2 A22)} for the block preconditioner of the sub-options (pph_mg_smooth
    honoured).  An LU block (the direct-equivalent solve included) means the block solve is exact: its value is 1.0, returned
    without touching the device.  pc_type none and a block pc_type none raise NotImplementedError."""
    from .forms import dpp_form
    from .solver import translate_options

    cfg, _info = translate_options(solver_parameters, nonlinear=nonlinear)
    names = {v: k for k, v in _PC_NAMES.items()}
    split = bool(cfg.picard) or cfg.pc_type == _ffi.PC_FIELDSPLIT
    if split and cfg.inner_exact:
        return {"macro": 1.0, "micro": 1.0}
    pc = cfg.inner_pc_type if split else cfg.pc_type
    pc_name = names.get(pc, "none")
    _check_preconditioned_pairing(not split, W, pc_name)
    a, _L = dpp_form(W, params)
    ctx, _which = _assemble_for(a, bcs)
    ns = int(cfg.mg_smooth) if cfg.mg_smooth > 0 else 2
    if not split:
        return {"monolithic": _pc_kappa(ctx, _ffi.MAT_MONO, pc_name, ns, tol)}
    return {"macro": _pc_kappa(ctx, _ffi.MAT_A11, pc_name, ns, tol), "micro": _pc_kappa(ctx, _ffi.MAT_A22, pc_name, ns, tol)}


class _FieldView(fd.FunctionSpace):
    def __init__(self, V, field):
        super().__init__(V.mesh(), "CG", getattr(V, "degree", 1))
        self.index = field


def _as_field(bc: fd.DirichletBC, field: int):
    return _FieldView(bc.function_space(), field)


def assemble_bilinear_form(form, boundary_conditions: List[fd.DirichletBC]):
    """The assembled operator of `form` with the BCs applied (reference conditioning.py:51-63 returns the Firedrake
    matrix; here: the SciPy CSR exported from the device, explicit zeros of the eliminated pattern kept, like a
    PETSc aij matrix)."""
    if isinstance(form, DPPBilinearForm):
        ctx = _context(form.space)
        _set_bcs(ctx, form.space, boundary_conditions)
        ctx.assemble(form.k1, form.k2, form.beta, form.mu, monolithic=True)
        return csr_matrix(ctx.csr(_ffi.MAT_MONO))
    return get_matrix_data_from_form(form, boundary_conditions).sparse_csr_data


def _dense_singular_values(A: csr_matrix) -> np.ndarray:
    return np.linalg.svd(A.toarray(), compute_uv=False)


def _extreme_singular_values(A: csr_matrix):
    """sigma_max and sigma_min without the full spectrum, in the order of the reference's sparse branch
    (conditioning.py:155-205): sigma_max from ARPACK `svds(which="LM")`; sigma_min from `svds(which="SM", tol=1e-8)`,
    failing that from the smallest eigenvalue of the normal equations A^T A (`eigsh(which="SM")`), failing that from a
    dense SVD - and any failure of the sigma_max call falls back to a dense SVD as well.  Returns (nan, None) semantics
    like the reference: sigma_min None when every route failed."""
    from scipy.sparse.linalg import eigsh, svds

    A = A.astype(np.float64)
    try:
        smax = float(np.max(svds(A, k=1, which="LM", maxiter=10000, return_singular_vectors=False, solver="arpack")))
    except Exception:
        sv = _dense_singular_values(A)
        smax = float(sv.max()) if sv.size else float("nan")
    smin = None
    try:
        smin = float(np.min(svds(A, k=1, which="SM", maxiter=20000, return_singular_vectors=False, solver="arpack", tol=1e-8)))
    except Exception:
        try:
            lam = eigsh((A.T @ A), k=1, which="SM", return_eigenvectors=False)
            smin = float(np.sqrt(max(float(lam[0]), 0.0)))
        except Exception:
            sv = _dense_singular_values(A)
            if sv.size:
                smin = float(sv.min())
    return smax, smin


def calculate_condition_number(scipy_csr_sparse_matrix: csr_matrix, num_singular_values: Optional[int] = None,
                               use_sparse: bool = False, zero_tol: float = DEFAULT_CONDITION_NUMBER_TOLERANCE,
                               num_of_factors: Optional[int] = None) -> float:
    """sigma_max / sigma_min over singular values above `zero_tol` (reference conditioning.py:105-218).  Dense SVD
    unless `use_sparse` with a positive `num_singular_values` (alias `num_of_factors`) below min(shape) - 1: then only
    the two extreme singular values are computed iteratively, as in the reference's sparse branch (:155-218; inf when
    the smallest one does not exceed the tolerance)."""
    A = scipy_csr_sparse_matrix
    k = num_singular_values if num_singular_values is not None else num_of_factors
    nmin = min(A.shape)
    if nmin == 0:
        return float("nan")
    if use_sparse and k is not None and 0 < int(k) < nmin - 1:
        smax, smin = _extreme_singular_values(csr_matrix(A))
        if smin is None or not np.isfinite(smax):
            return float("nan")
        return float("inf") if smin <= zero_tol else float(smax / smin)
    s = np.linalg.svd(A.toarray() if hasattr(A, "toarray") else np.asarray(A), compute_uv=False)
    s = s[s > zero_tol]
    if s.size == 0:
        return float("inf")
    return float(s.max() / s.min())
