"""
ctypes binding of ``libperphil_hip.so`` (C ABI declared in ``include/perphil_hip.h``).

This is the only crossing between the Python host layer and the device code: Python -> ctypes ->
C ABI -> HIP.  There is no CPU fallback: if the shared library is missing or cannot be loaded the
import of this module raises, and every call that fails inside the library raises
(``ValueError`` for PPH_ERR_INVALID, ``MemoryError`` for PPH_ERR_NOMEM, ``RuntimeError``
otherwise), mirroring how PETSc errors surface as exceptions from the reference's
``solver.solve()`` (reference ``src/perphil/solvers/solver.py:71``).
"""
from __future__ import annotations

import sys
import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PERPHIL_HIP_LIB") or os.path.join(_HERE, "libperphil_hip.so")   # (the override: A/B builds of tools/)

PPH_OK, PPH_ERR_INVALID, PPH_ERR_HIP, PPH_ERR_NOMEM, PPH_ERR_DIVERGED, PPH_ERR_COMM = 0, -1, -2, -3, -4, -5
CELL_QUAD, CELL_TRI, CELL_HEX, CELL_TET = 0, 1, 2, 3
KSP_PREONLY, KSP_CG, KSP_GMRES = 0, 1, 2
PC_NONE, PC_JACOBI, PC_BLOCK2, PC_FIELDSPLIT, PC_MG, PC_ILU, PC_PMG, PC_CMG = 0, 1, 2, 3, 4, 5, 6, 7
MAT_MONO, MAT_K, MAT_M, MAT_A11, MAT_A22, MAT_A12, MAT_A21 = 0, 1, 2, 3, 4, 5, 6

# every symbol include/perphil_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "pph_ctx_create", "pph_ctx_destroy", "pph_last_error", "pph_ctx_synchronize",
    "pph_mesh_build", "pph_mesh_build_lagrange", "pph_mesh_sizes", "pph_get_dofmap", "pph_get_coords",
    "pph_set_dirichlet", "pph_assemble_dpp",
    "pph_solve", "pph_solve_device", "pph_get_solution", "pph_host_alloc", "pph_host_free",
    "pph_csr_sizes", "pph_get_csr", "pph_get_rhs", "pph_spmv", "pph_spmv_bench",
    "pph_get_timers", "pph_set_option", "pph_comm_set_callbacks",
    "pph_rccl_available", "pph_rccl_unique_id", "pph_comm_init_rccl", "pph_comm_selftest", "pph_comm_selftest2",
    "pph_comm_stats", "pph_comm_times", "pph_error_norms_mms", "pph_quadrature_points", "pph_error_norms_sampled", "pph_bw_probe",
    "pph_darcy_velocity",
    "pph_get_stream", "pph_copy_solution_device", "pph_set_dirichlet_device", "pph_error_norms_mms_device",
    "pph_error_norms_sampled_device", "pph_darcy_velocity_device",
    "pph_pc_apply", "pph_pc_bench", "pph_asm_wave_map", "pph_pc_apply_coupled", "pph_cmg_bench",
    "pph_eval_points", "pph_eval_points_device",
    "pph_integrate", "pph_integrate_device", "pph_boundary_flux", "pph_boundary_flux_device",
    "pph_dpp_nodal_flux", "pph_dpp_nodal_flux_device",
    "pph_extreme_eigenvalues", "pph_tridiag_extremes", "pph_preconditioned_extremes",
    "pph_trace_pathlines", "pph_trace_pathlines_device",
    "pph_solve_rhs", "pph_solve_rhs_device", "pph_dpp_bilinear", "pph_dpp_bilinear_device",
    "pph_dpp_step_rhs", "pph_dpp_step_rhs_device", "pph_assemble_dpp_shifted",
    "pph_transient_begin", "pph_transient_steps", "pph_transient_steps_device",
    "pph_transient_steps_record", "pph_transient_steps_record_device",
    "pph_transient_bilinear", "pph_transient_bilinear_device", "pph_eval_points_adjoint", "pph_eval_points_adjoint_device",
    "pph_transient_adjoint", "pph_transient_adjoint_device",
    "pph_sources_set", "pph_sources_set_device", "pph_sources_clear", "pph_sources_count",
    "pph_sources_apply", "pph_sources_apply_device", "pph_transient_steps_sources", "pph_transient_steps_sources_device",
    "pph_transient_adjoint_sources", "pph_transient_adjoint_sources_device",
]

HALO_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)


class _PinnedBlock:
    """Owner of one pph_host_alloc block; freed when the last NumPy array over it is gone."""

    def __init__(self, ptr: int):
        self.ptr = ptr

    def __del__(self):
        try:
            if self.ptr:
                lib.pph_host_free(C.c_void_p(self.ptr))
                self.ptr = 0
        except Exception:
            pass


def _pinned_array(n: int):
    """float64[n] over page-locked memory, or None when the allocation fails."""
    out = C.c_void_p()
    if lib.pph_host_alloc(C.c_size_t(8 * n), C.byref(out)) != 0 or not out.value:
        return None
    cbuf = (C.c_double * n).from_address(out.value)
    cbuf._owner = _PinnedBlock(out.value)     # the ctypes array is the base of every NumPy view: it keeps the block alive
    return np.frombuffer(cbuf, dtype=np.float64, count=n)


class SolverCfg(C.Structure):
    """``pph_solver_cfg``"""
    _fields_ = [
        ("ksp_type", C.c_int32), ("pc_type", C.c_int32), ("restart", C.c_int32), ("max_it", C.c_int32),
        ("rtol", C.c_double), ("atol", C.c_double),
        ("inner_ksp_type", C.c_int32), ("inner_pc_type", C.c_int32), ("inner_max_it", C.c_int32),
        ("picard", C.c_int32),
        ("inner_rtol", C.c_double), ("inner_atol", C.c_double),
        ("picard_rtol", C.c_double), ("picard_atol", C.c_double),
        ("picard_max_it", C.c_int32), ("mg_smooth", C.c_int32),
        ("inner_reduction", C.c_double),
        ("inner_norm", C.c_int32), ("inner_exact", C.c_int32),
    ]


class SolveInfo(C.Structure):
    """``pph_solve_info``"""
    _fields_ = [
        ("iterations", C.c_int32), ("inner_iterations", C.c_int32), ("converged", C.c_int32),
        ("inner_failed", C.c_int32), ("resnorm", C.c_double), ("rhs_norm", C.c_double),
    ]


def _preload_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so / libhsa-runtime64.so
    (same SONAMEs as /opt/rocm's, loaded by path): if this library binds the system copy first and torch
    is imported later, two runtimes coexist and the second one finds no GPU.  So when torch is installed
    and not yet imported, its copy is loaded first (RTLD_GLOBAL) and libperphil_hip.so resolves its
    libamdhip64.so.7 dependency to it.  PERPHIL_HIP_RUNTIME=system skips this."""
    import importlib.util
    import sys

    if "torch" in sys.modules or os.environ.get("PERPHIL_HIP_RUNTIME", "") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def _load() -> C.CDLL:
    _preload_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C perphil_amd/csrc`).  perphil_amd has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    p = C.c_void_p
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    sig = {
        "pph_ctx_create": ([C.c_int, C.POINTER(p)], C.c_int),
        "pph_ctx_destroy": ([p], C.c_int),
        "pph_last_error": ([p], C.c_char_p),
        "pph_ctx_synchronize": ([p], C.c_int),
        "pph_mesh_build": ([p] + [C.c_int] * 9, C.c_int),
        "pph_mesh_build_lagrange": ([p] + [C.c_int] * 6, C.c_int),
        "pph_mesh_sizes": ([p, i64p, i64p, i32p, i64p], C.c_int),
        "pph_get_dofmap": ([p, C.c_void_p], C.c_int),
        "pph_get_coords": ([p, C.c_void_p], C.c_int),
        "pph_set_dirichlet": ([p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
        "pph_assemble_dpp": ([p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int], C.c_int),
        "pph_solve": ([p, C.POINTER(SolverCfg), C.c_void_p, C.POINTER(SolveInfo), C.c_void_p, C.c_int], C.c_int),
        "pph_solve_device": ([p, C.POINTER(SolverCfg), C.POINTER(SolveInfo), C.c_void_p, C.c_int], C.c_int),
        "pph_get_solution": ([p, C.c_void_p], C.c_int),
        "pph_host_alloc": ([C.c_size_t, C.POINTER(C.c_void_p)], C.c_int),
        "pph_host_free": ([C.c_void_p], C.c_int),
        "pph_csr_sizes": ([p, C.c_int, i64p, i64p], C.c_int),
        "pph_get_csr": ([p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
        "pph_get_rhs": ([p, C.c_void_p, C.c_void_p], C.c_int),
        "pph_spmv": ([p, C.c_int, C.c_void_p, C.c_void_p], C.c_int),
        "pph_spmv_bench": ([p, C.c_int, C.c_int, f64p], C.c_int),
        "pph_get_timers": ([p, C.c_void_p, C.c_int], C.c_int),
        "pph_set_option": ([p, C.c_char_p, C.c_double], C.c_int),
        "pph_comm_set_callbacks": ([p, C.c_int, C.c_int, HALO_FN, ALLREDUCE_FN, C.c_void_p], C.c_int),
        "pph_rccl_unique_id": ([C.c_char_p, C.c_void_p], C.c_int),
        "pph_comm_init_rccl": ([p, C.c_int, C.c_int, C.c_void_p, C.c_char_p], C.c_int),
        "pph_comm_selftest": ([p], C.c_int),
        "pph_comm_selftest2": ([p, C.POINTER(C.c_int)], C.c_int),
        "pph_comm_stats": ([p, i64p, i64p, C.POINTER(C.c_int)], C.c_int),
        "pph_comm_times": ([p, f64p], C.c_int),
        "pph_rccl_available": ([C.c_char_p], C.c_int),
        "pph_bw_probe": ([p, C.c_int64, C.c_int, C.c_int, f64p], C.c_int),
        "pph_error_norms_mms": ([p, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, f64p,
                                 f64p], C.c_int),
        "pph_darcy_velocity": ([p, C.c_void_p, C.c_double, C.c_void_p], C.c_int),
        "pph_quadrature_points": ([p, C.c_int, C.c_int64, C.c_int64, C.c_void_p], C.c_int),
        "pph_error_norms_sampled": ([p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, f64p, f64p], C.c_int),
        "pph_get_stream": ([p, C.POINTER(C.c_void_p)], C.c_int),
        "pph_copy_solution_device": ([p, C.c_void_p, C.c_int64], C.c_int),
        "pph_set_dirichlet_device": ([p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
        "pph_error_norms_mms_device": ([p, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                                        f64p, f64p], C.c_int),
        "pph_error_norms_sampled_device": ([p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                            f64p, f64p], C.c_int),
        "pph_darcy_velocity_device": ([p, C.c_void_p, C.c_double, C.c_void_p], C.c_int),
        "pph_pc_apply": ([p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p], C.c_int),
        "pph_pc_bench": ([p, C.c_int, C.c_int, C.c_int, C.c_int, f64p], C.c_int),
        "pph_pc_apply_coupled": ([p, C.c_int, C.c_int, C.c_void_p, C.c_void_p], C.c_int),
        "pph_cmg_bench": ([p, C.c_int, C.c_int, f64p], C.c_int),
        "pph_asm_wave_map": ([C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, i64p], C.c_int),
        "pph_eval_points": ([p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, i64p], C.c_int),
        "pph_eval_points_device": ([p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, i64p],
                                   C.c_int),
        "pph_integrate": ([p, C.c_void_p, f64p], C.c_int),
        "pph_integrate_device": ([p, C.c_void_p, f64p], C.c_int),
        "pph_boundary_flux": ([p, C.c_void_p, C.c_double, f64p], C.c_int),
        "pph_boundary_flux_device": ([p, C.c_void_p, C.c_double, f64p], C.c_int),
        "pph_dpp_nodal_flux": ([p] + [C.c_double] * 4 + [C.c_void_p, C.c_void_p], C.c_int),
        "pph_dpp_nodal_flux_device": ([p] + [C.c_double] * 4 + [C.c_void_p, C.c_void_p], C.c_int),
        "pph_extreme_eigenvalues": ([p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, f64p], C.c_int),
        "pph_tridiag_extremes": ([C.c_void_p, C.c_void_p, C.c_int, f64p], C.c_int),
        "pph_preconditioned_extremes": ([p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, f64p], C.c_int),
        "pph_trace_pathlines": ([p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_double, C.c_int32,
                                 C.c_int32] + [C.c_void_p] * 6 + [i64p], C.c_int),
        "pph_trace_pathlines_device": ([p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_double,
                                        C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [i64p], C.c_int),
        "pph_solve_rhs": ([p, C.POINTER(SolverCfg), C.c_void_p, C.c_void_p, C.POINTER(SolveInfo), C.c_void_p, C.c_int], C.c_int),
        "pph_solve_rhs_device": ([p, C.POINTER(SolverCfg), C.c_void_p, C.c_void_p, C.POINTER(SolveInfo), C.c_void_p, C.c_int],
                                 C.c_int),
        "pph_dpp_bilinear": ([p, C.c_void_p, C.c_void_p, f64p], C.c_int),
        "pph_dpp_bilinear_device": ([p, C.c_void_p, C.c_void_p, f64p], C.c_int),
        "pph_dpp_step_rhs": ([p] + [C.c_double] * 4 + [C.c_void_p, C.c_void_p], C.c_int),
        "pph_dpp_step_rhs_device": ([p] + [C.c_double] * 4 + [C.c_void_p, C.c_void_p], C.c_int),
        "pph_assemble_dpp_shifted": ([p] + [C.c_double] * 6 + [C.c_int], C.c_int),
        "pph_transient_begin": ([p] + [C.c_double] * 8 + [C.c_int], C.c_int),
        "pph_transient_steps": ([p, C.POINTER(SolverCfg), C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_int)], C.c_int),
        "pph_transient_steps_device": ([p, C.POINTER(SolverCfg), C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_int)], C.c_int),
        "pph_transient_steps_record": ([p, C.POINTER(SolverCfg), C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_int), C.c_void_p], C.c_int),
        "pph_transient_steps_record_device": ([p, C.POINTER(SolverCfg), C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                               C.POINTER(C.c_int), C.c_void_p], C.c_int),
        "pph_transient_bilinear": ([p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, f64p], C.c_int),
        "pph_transient_bilinear_device": ([p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, f64p], C.c_int),
        "pph_eval_points_adjoint": ([p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_void_p, i64p], C.c_int),
        "pph_eval_points_adjoint_device": ([p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_void_p, i64p], C.c_int),
        "pph_transient_adjoint": ([p, C.POINTER(SolverCfg)] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_double, C.c_int]
                                  + [C.c_void_p] * 4 + [C.POINTER(C.c_int)], C.c_int),
        "pph_transient_adjoint_device": ([p, C.POINTER(SolverCfg)] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_double, C.c_int]
                                         + [C.c_void_p] * 4 + [C.POINTER(C.c_int)], C.c_int),
        "pph_sources_set": ([p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, i64p], C.c_int),
        "pph_sources_set_device": ([p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, i64p], C.c_int),
        "pph_sources_clear": ([p], C.c_int),
        "pph_sources_count": ([p, i64p], C.c_int),
        "pph_sources_apply": ([p, C.c_void_p, C.c_void_p], C.c_int),
        "pph_sources_apply_device": ([p, C.c_void_p, C.c_void_p], C.c_int),
        "pph_transient_steps_sources": ([p, C.POINTER(SolverCfg), C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
        "pph_transient_steps_sources_device": ([p, C.POINTER(SolverCfg), C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
        "pph_transient_adjoint_sources": ([p, C.POINTER(SolverCfg)] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_double, C.c_int]
                                          + [C.c_void_p] * 4 + [C.POINTER(C.c_int), C.c_void_p, C.c_int64], C.c_int),
        "pph_transient_adjoint_sources_device": ([p, C.POINTER(SolverCfg)] + [C.c_void_p] * 3
                                                 + [C.c_int64, C.c_void_p, C.c_double, C.c_int] + [C.c_void_p] * 4
                                                 + [C.POINTER(C.c_int), C.c_void_p, C.c_int64], C.c_int),
    }
    for name, (argtypes, restype) in sig.items():
        fn = getattr(lib, name)  # AttributeError here = ABI mismatch: fail loudly
        fn.argtypes = argtypes
        fn.restype = restype
    return lib


lib = _load()


def tridiag_extremes(alpha, beta) -> tuple:
    """(theta_min, theta_max, last component of either normalised eigenvector) of the symmetric tridiagonal matrix with
    diagonal `alpha` [m] and off-diagonal `beta` [m - 1]: the host routine behind the Lanczos checks (no device touched)."""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    if alpha.ndim != 1 or alpha.size < 1 or beta.shape != (alpha.size - 1,):
        raise ValueError("tridiag_extremes: alpha [m >= 1] and beta [m - 1]")
    out = (C.c_double * 4)()
    st = lib.pph_tridiag_extremes(_ptr(alpha), _ptr(beta) if beta.size else None, int(alpha.size), out)
    if st != PPH_OK:
        raise ValueError((lib.pph_last_error(None) or b"").decode())
    return out[0], out[1], out[2], out[3]


class ConvergenceError(RuntimeError):
    """Krylov / Picard iteration did not converge (Firedrake raises ConvergenceError likewise)."""


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# -- device-resident results ------------------------------------------------------------------------
# Torch tensors and this library share one HIP runtime when torch's copy of it was loaded first (_preload_hip_runtime):
# device pointers then cross freely and results can stay in GPU memory.  With PERPHIL_HIP_RUNTIME=system, without torch,
# or when two runtimes ended up in the process anyway, they cannot: results are copied to the host as before.
_shared: Optional[bool] = None

# solution-sized device-to-host copies made so far (solves with fetch, Context.solution, first host access of a
# device-resident fd.Function): what a caller who keeps results on the device should see stay at zero
fetch_stats = {"fetches": 0, "bytes": 0}


def _count_fetch(nbytes: int) -> None:
    fetch_stats["fetches"] += 1
    fetch_stats["bytes"] += int(nbytes)


def shared_runtime() -> bool:
    """True when torch's device tensors and this library's device pointers belong to one HIP runtime."""
    global _shared
    if _shared is None:
        _shared = _probe_shared_runtime()
    return _shared


def _probe_shared_runtime() -> bool:
    if os.environ.get("PERPHIL_HIP_RUNTIME", "") == "system":
        return False
    try:
        import torch
    except ImportError:
        return False
    if not getattr(torch.version, "hip", None):
        return False
    try:
        with open("/proc/self/maps") as f:
            libs = {os.path.realpath(line.split()[-1]) for line in f if "libamdhip64.so" in line}
    except OSError:
        libs = set()
    return len(libs) <= 1


def require_shared_runtime(what: str) -> None:
    if not shared_runtime():
        raise RuntimeError(f"{what} needs torch and this library on one HIP runtime (torch installed, imported through "
                           "perphil_amd's preload, PERPHIL_HIP_RUNTIME not 'system'); copy the data to the host instead")


def _tptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def tensor_to_host(t, ctx: Optional["Context"] = None) -> np.ndarray:
    """float64 device tensor -> NumPy array (the context's pinned result pool for large ones), on torch's current stream."""
    import torch

    n = t.numel()
    arr = ctx._result_array(n) if ctx is not None else np.empty(n, dtype=np.float64)
    torch.from_numpy(arr).copy_(t.reshape(-1))
    _count_fetch(8 * n)
    return arr


class Context:
    """Owner of one ``pph_ctx`` (one GPU, one stream).  Not thread-safe; one per device."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        st = lib.pph_ctx_create(int(device), C.byref(self._h))
        if st != PPH_OK:
            msg = (lib.pph_last_error(None) or b"").decode()
            raise RuntimeError(f"pph_ctx_create(device={device}) failed ({st}): {msg}")
        self.device = int(device)
        self.n = 0
        self.dim = 0
        self._bc_state = {}

    # -- plumbing -----------------------------------------------------------------------------
    def _check(self, st: int, allow_diverged: bool = False) -> int:
        if st == PPH_OK or (allow_diverged and st == PPH_ERR_DIVERGED):
            return st
        msg = (lib.pph_last_error(self._h) or b"").decode()
        if st == PPH_ERR_INVALID:
            raise ValueError(msg)
        if st == PPH_ERR_NOMEM:
            raise MemoryError(msg)
        if st == PPH_ERR_DIVERGED:
            raise ConvergenceError(msg)
        raise RuntimeError(f"libperphil_hip error {st}: {msg}")

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            lib.pph_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self) -> None:
        self._check(lib.pph_ctx_synchronize(self._h))

    def set_option(self, name: str, value: float) -> None:
        self._check(lib.pph_set_option(self._h, name.encode(), float(value)))

    # -- mesh ---------------------------------------------------------------------------------
    def mesh_build(self, dim: int, kind: int, nx: int, ny: int, nz: int = 0, z_begin: int = 0,
                   z_count: Optional[int] = None, ghost_lo: bool = False, ghost_hi: bool = False) -> None:
        if z_count is None:
            z_count = nz
        self._check(lib.pph_mesh_build(self._h, dim, kind, nx, ny, nz, z_begin, z_count, int(ghost_lo), int(ghost_hi)))
        n, nc, m, nnz = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
        self._check(lib.pph_mesh_sizes(self._h, C.byref(n), C.byref(nc), C.byref(m), C.byref(nnz)))
        self.n, self.ncell, self.m, self.nnzb, self.dim = n.value, nc.value, m.value, nnz.value, dim
        self._bc_state = {}
        # cells of the device norms (pph_error_norms_*_device): a slab leaves the layer above its lower ghost plane to the
        # neighbour that owns the plane
        self._slab_cells = (self.ncell // z_count if ghost_lo and dim == 3 else 0, self.ncell)

    def mesh_build_lagrange(self, dim: int, kind: int, nx: int, ny: int, nz: int = 0, degree: int = 2) -> None:
        """Whole mesh with Lagrange nodes of `degree` (1 or 2; degree 2: the lattice refined once, CSR operators only)."""
        self._check(lib.pph_mesh_build_lagrange(self._h, dim, kind, nx, ny, nz, int(degree)))
        n, nc, m, nnz = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
        self._check(lib.pph_mesh_sizes(self._h, C.byref(n), C.byref(nc), C.byref(m), C.byref(nnz)))
        self.n, self.ncell, self.m, self.nnzb, self.dim = n.value, nc.value, m.value, nnz.value, dim
        self.degree = int(degree)
        self._bc_state = {}
        self._slab_cells = (0, self.ncell)

    def dofmap(self) -> np.ndarray:
        out = np.empty((self.ncell, self.m), dtype=np.int32)
        self._check(lib.pph_get_dofmap(self._h, _ptr(out)))
        return out

    def coords(self) -> np.ndarray:
        out = np.empty((self.n, self.dim), dtype=np.float64)
        self._check(lib.pph_get_coords(self._h, _ptr(out)))
        return out

    # -- system -------------------------------------------------------------------------------
    def set_dirichlet(self, field: int, nodes: np.ndarray, vals: np.ndarray) -> None:
        nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if nodes.shape != vals.shape:
            raise ValueError("nodes and vals must have the same shape")
        self._check(lib.pph_set_dirichlet(self._h, int(field), _ptr(nodes), _ptr(vals), nodes.size))
        self._bc_state[int(field)] = (nodes.copy(), vals.copy())

    def same_dirichlet(self, field: int, nodes, vals) -> bool:
        """True when exactly this set (nodes and values) is what the device holds for `field` (callers skip the
        upload then: pph_set_dirichlet drops the assembled system and makes the multigrid levels re-derive their masks).
        Device tensors are compared on the device with the set a tensor call left; a host set and a device set are
        never taken for the same one (the set is applied again)."""
        old = self._bc_state.get(int(field))
        if old is None:
            return False
        if isinstance(old[1], np.ndarray) != isinstance(vals, np.ndarray):
            return False
        if isinstance(vals, np.ndarray):
            return (np.array_equal(old[0], np.asarray(nodes, dtype=np.int64))
                    and np.array_equal(old[1], np.asarray(vals, dtype=np.float64)))
        import torch

        return (old[0].shape == nodes.shape and old[1].shape == vals.shape and torch.equal(old[0], nodes)
                and torch.equal(old[1], vals))

    def assemble(self, k1: float, k2: float, beta: float, mu: float, monolithic: bool = True, sigma=(0.0, 0.0),
                 shifted_entry: bool = False) -> None:
        """Assembles the eliminated blocks and the lifted right-hand side; ``sigma`` = (sigma1, sigma2) adds sigma_f M to the
        diagonal block of field f (pph_assemble_dpp_shifted; (0, 0) is pph_assemble_dpp itself, unless ``shifted_entry`` asks
        for the shifted entry point whatever sigma is)."""
        s1, s2 = (float(v) for v in sigma)
        if s1 == 0.0 and s2 == 0.0 and not shifted_entry:
            self._check(lib.pph_assemble_dpp(self._h, float(k1), float(k2), float(beta), float(mu), int(monolithic)))
        else:
            self._check(lib.pph_assemble_dpp_shifted(self._h, float(k1), float(k2), float(beta), float(mu), s1, s2,
                                                     int(monolithic)))

    # -- result vectors ---------------------------------------------------------------------
    # Large results land in page-locked host arrays: the device-to-host copy then runs at PCIe speed and no fresh pages
    # are touched (256^3: 5 - 6 ms instead of 15 - 27 for the 272 MB solution).  The arrays are ordinary NumPy arrays whose
    # memory belongs to a _PinnedBlock that frees it when the last array / view of it dies; a pool of up to three blocks
    # per context hands out a block again once nobody but the pool refers to its array (a loop that overwrites `sol` each
    # time alternates between two blocks); a caller that keeps more than three results alive gets pageable arrays.
    _PIN_MIN = 1 << 20      # entries; smaller results use pageable arrays
    _PIN_POOL = 3

    @staticmethod
    def _idle_refcount() -> int:
        # what sys.getrefcount reports for an object only a list refers to, counted the way _result_array counts (list entry,
        # loop variable, the call's argument): measured on this interpreter instead of assumed (3 on CPython 3.10)
        for o in [object()]:
            return sys.getrefcount(o)
        return 3

    def _result_array(self, n: int) -> np.ndarray:
        if n < self._PIN_MIN:
            return np.empty(n, dtype=np.float64)
        pool = self.__dict__.setdefault("_pinned", [])
        idle = self.__dict__.setdefault("_pinned_idle", self._idle_refcount())
        for arr in pool:
            if arr.shape[0] == n and sys.getrefcount(arr) <= idle:    # nobody but the pool refers to it (views count: their base is arr)
                return arr
        pool[:] = [a for a in pool if a.shape[0] == n]
        if len(pool) >= self._PIN_POOL:
            return np.empty(n, dtype=np.float64)
        arr = _pinned_array(n)
        if arr is None:
            return np.empty(n, dtype=np.float64)
        pool.append(arr)
        if len(pool) == 1:
            # the usual caller overwrites its previous result with the next: that needs two blocks - pin both now (17 ms
            # each at 272 MB) rather than inside the second, typically timed, call
            second = _pinned_array(n)
            if second is not None:
                pool.append(second)
        return arr

    def solve(self, cfg: SolverCfg, fetch: bool = True, hist_cap: int = 0, raise_on_diverged: bool = True):
        info = SolveInfo()
        hist = np.zeros(max(hist_cap, 1), dtype=np.float64)
        x = self._result_array(2 * self.n) if fetch else None
        if fetch:
            _count_fetch(8 * x.size)
            st = lib.pph_solve(self._h, C.byref(cfg), _ptr(x), C.byref(info), _ptr(hist), int(hist_cap))
        else:
            st = lib.pph_solve_device(self._h, C.byref(cfg), C.byref(info), _ptr(hist), int(hist_cap))
        self.last_info = info        # (what the solve reported, also when the status below raises)
        self._check(st, allow_diverged=not raise_on_diverged)
        nh = min(hist_cap, info.iterations + 1)
        return x, info, hist[:nh].copy()

    def solution(self) -> np.ndarray:
        x = self._result_array(2 * self.n)
        self._check(lib.pph_get_solution(self._h, _ptr(x)))
        _count_fetch(8 * x.size)
        return x

    # -- device-resident results (torch tensors; shared runtime only) -------------------------
    def torch_device(self):
        import torch

        return torch.device("cuda", self.device)

    def torch_stream(self):
        """The context's stream as a ``torch.cuda.ExternalStream``."""
        st = self.__dict__.get("_tstream")
        if st is None or self.__dict__.get("_tstream_h") != self._h.value:
            import torch

            require_shared_runtime("a device-resident result")
            ptr = C.c_void_p()
            self._check(lib.pph_get_stream(self._h, C.byref(ptr)))
            st = torch.cuda.ExternalStream(ptr.value, device=self.torch_device())
            self._tstream, self._tstream_h = st, self._h.value
        return st

    def wait_for_torch(self) -> None:
        """Torch -> library: the context stream waits for the work torch has enqueued so far (no host wait)."""
        import torch

        self.torch_stream().wait_stream(torch.cuda.current_stream(self.torch_device()))

    def torch_waits(self) -> None:
        """Library -> torch: torch's current stream waits for the work enqueued on the context stream so far."""
        import torch

        torch.cuda.current_stream(self.torch_device()).wait_stream(self.torch_stream())

    # Blocks of torch's allocator and the context stream: no record_stream on the context stream - the allocator would
    # record an event on that stream when the tensor dies, which may be after close() destroyed the stream.  Instead every
    # entry point that writes a tensor is followed at once by torch_waits() (torch's current stream, the block's own, waits
    # for the write: a block freed later is reused after it), and every entry point that reads one returns only after the
    # context stream has finished reading (it synchronises).
    def _device_out(self, n: int):
        """A fresh float64 tensor of torch's caching allocator for the context stream to write into (call torch_waits()
        right after the write)."""
        import torch

        t = torch.empty(n, dtype=torch.float64, device=self.torch_device())
        self.wait_for_torch()                  # (the block may still be read by torch work enqueued earlier)
        return t

    def _device_in(self, t, n: int, name: str):
        """Checks a caller's device tensor and orders the context stream after torch's work on it."""
        import torch

        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.is_cuda and t.shape == (n,)
                and t.is_contiguous() and t.device.index == self.device):
            raise ValueError(f"{name} must be a contiguous float64 tensor of {n} values on cuda:{self.device}")
        self.wait_for_torch()
        return t

    def solution_tensor(self):
        """The current solution copied (on the device) into a new torch tensor; torch's current stream is ordered after it."""
        t = self._device_out(2 * self.n)
        self._check(lib.pph_copy_solution_device(self._h, _tptr(t), t.numel()))
        self.torch_waits()
        return t

    def set_dirichlet_device(self, field: int, nodes, vals) -> None:
        """pph_set_dirichlet from device tensors (int64 nodes, float64 values)."""
        import torch

        if nodes.dtype != torch.int64 or not nodes.is_cuda or nodes.dim() != 1 or not nodes.is_contiguous():
            raise ValueError("nodes must be a contiguous int64 tensor on the device")
        vals = self._device_in(vals, nodes.numel(), "vals")
        self._check(lib.pph_set_dirichlet_device(self._h, int(field), _tptr(nodes), _tptr(vals), nodes.numel()))
        self._bc_state[int(field)] = (nodes.clone(), vals.clone())

    def error_norms_mms_device(self, field: int, nodal, k1: float, k2: float, beta: float, mu: float, nq: int = 6):
        """error_norms_mms of a device tensor (collective on a slab: owned cells, summed over the ranks)."""
        nodal = self._device_in(nodal, self.n, "nodal field")
        l2, h1 = C.c_double(), C.c_double()
        self._check(lib.pph_error_norms_mms_device(self._h, int(field), _tptr(nodal), float(k1), float(k2), float(beta),
                                                   float(mu), int(nq), C.byref(l2), C.byref(h1)))
        return l2.value, h1.value

    def owned_cells(self) -> tuple:
        """[begin, end) of the cells this context integrates over in the device norms (all of them on a single context)."""
        s = self.__dict__.get("_slab_cells")
        return s if s is not None else (0, self.ncell)

    def error_norms_sampled_device(self, nodal, exact, grad=None, nq: int = 6, chunk_cells: int = 1 << 16):
        """error_norms_sampled of a device tensor, over this context's owned cells in chunks (collective on a slab: the
        field's ghost planes are refreshed by the first call, the sums are reduced over the ranks by the last)."""
        nodal = self._device_in(nodal, self.n, "nodal field")
        c0, c1 = self.owned_cells()
        if exact is None:
            chunk_cells = max(c1 - c0, 1)
        starts = list(range(c0, c1, chunk_cells)) or [c1]
        a, b = C.c_double(), C.c_double()
        for k, b0 in enumerate(starts):
            cnt = min(chunk_cells, c1 - b0)
            se = sg = None
            if exact is not None and cnt > 0:
                se, sg = self._samples(exact, grad, nq, b0, cnt)
            self._check(lib.pph_error_norms_sampled_device(self._h, _tptr(nodal) if k == 0 else None, int(nq), int(b0),
                                                           int(cnt), _ptr(se), _ptr(sg), int(k == len(starts) - 1),
                                                           C.byref(a), C.byref(b)))
        return float(np.sqrt(a.value)), float(np.sqrt(b.value))

    def darcy_velocity_device(self, nodal, conductivity: float):
        """darcy_velocity of a device tensor; returns a device tensor [n * dim] (node-major)."""
        nodal = self._device_in(nodal, self.n, "pressure")
        out = self._device_out(self.n * self.dim)
        self._check(lib.pph_darcy_velocity_device(self._h, _tptr(nodal), float(conductivity), _tptr(out)))
        self.torch_waits()
        return out

    def eval_points_device(self, nodal, points, ncomp: int = 1, gradient: bool = False, tol: float = 1e-12):
        """eval_points on device tensors: nodal [n * ncomp], points [m, dim] -> (values [m, ncomp], gradients
        [m, ncomp, dim] or None, number of outside points), tensors on the device.  Nothing but the count moves to the host."""
        import torch

        nodal = self._device_in(nodal, self.n * int(ncomp), "nodal field")
        if not (isinstance(points, torch.Tensor) and points.dtype == torch.float64 and points.is_cuda and points.dim() == 2
                and points.shape[1] == self.dim and points.is_contiguous() and points.device.index == self.device):
            raise ValueError(f"points must be a contiguous float64 tensor [m, {self.dim}] on cuda:{self.device}")
        m = points.shape[0]
        val = self._device_out(m * int(ncomp)).reshape(m, int(ncomp))
        grad = self._device_out(m * int(ncomp) * self.dim).reshape(m, int(ncomp), self.dim) if gradient else None
        nout = C.c_int64()
        self._check(lib.pph_eval_points_device(self._h, _tptr(nodal), int(ncomp), _tptr(points), int(m), float(tol), _tptr(val),
                                               _tptr(grad) if gradient else None, C.byref(nout)))
        self.torch_waits()
        return val, grad, int(nout.value)

    def trace_pathlines_device(self, nodal, seeds, scale: float, dt: float, max_steps: int, min_speed: float = 0.0,
                               chunk: int = 4096, record_every: int = 0):
        """trace_pathlines on device tensors: nodal [n * dim], seeds [m, dim] -> (end [m, dim], time [m], length [m],
        steps [m] int32, status [m] int32 (status | side << 8), path [n_rec, m, dim] or None, counts [4]); tensors on the
        device.  Nothing but the counts moves to the host."""
        import torch

        nodal = self._device_in(nodal, self.n * self.dim, "nodal velocity")
        if not (isinstance(seeds, torch.Tensor) and seeds.dtype == torch.float64 and seeds.is_cuda and seeds.dim() == 2
                and seeds.shape[1] == self.dim and seeds.is_contiguous() and seeds.device.index == self.device):
            raise ValueError(f"seeds must be a contiguous float64 tensor [m, {self.dim}] on cuda:{self.device}")
        m = seeds.shape[0]
        n_rec = int(max_steps) // int(record_every) + 1 if record_every > 0 else 0
        end = self._device_out(m * self.dim).reshape(m, self.dim)
        time, length = self._device_out(m), self._device_out(m)
        steps = torch.empty(m, dtype=torch.int32, device=self.torch_device())
        status = torch.empty(m, dtype=torch.int32, device=self.torch_device())
        path = self._device_out(n_rec * m * self.dim).reshape(n_rec, m, self.dim) if n_rec else None
        self.wait_for_torch()
        counts = (C.c_int64 * 4)()
        self._check(lib.pph_trace_pathlines_device(self._h, _tptr(nodal), float(scale), _tptr(seeds), int(m), float(dt),
                                                   int(max_steps), float(min_speed), int(chunk), int(record_every), _tptr(end),
                                                   _tptr(time), _tptr(length), _tptr(steps), _tptr(status),
                                                   _tptr(path) if n_rec else None, counts))
        self.torch_waits()
        return end, time, length, steps, status, path, list(counts)

    # -- mass balance (pph_flux.hip): a NumPy array is uploaded for the call, a device tensor is read where it is ----
    def _nodal_arg(self, nodal, n: int, name: str):
        if isinstance(nodal, np.ndarray):
            a = np.ascontiguousarray(nodal, dtype=np.float64)
            if a.shape != (n,):
                raise ValueError(f"{name} must have {n} values, got {a.shape}")
            return a, _ptr(a), False
        return nodal, _tptr(self._device_in(nodal, n, name)), True

    def integrate(self, nodal) -> float:
        """int p_h dx of a nodal field of the context's space (pph_integrate / pph_integrate_device)."""
        keep, ptr, dev = self._nodal_arg(nodal, self.n, "nodal field")
        out = C.c_double()
        fn = lib.pph_integrate_device if dev else lib.pph_integrate
        self._check(fn(self._h, ptr, C.byref(out)))
        return out.value

    def boundary_flux(self, nodal, conductivity: float) -> np.ndarray:
        """F_s = int_{side s} -conductivity grad p_h . n ds, s = 1 .. 2 dim, as an array [2 dim] (pph_boundary_flux)."""
        keep, ptr, dev = self._nodal_arg(nodal, self.n, "nodal field")
        out = (C.c_double * 6)()
        fn = lib.pph_boundary_flux_device if dev else lib.pph_boundary_flux
        self._check(fn(self._h, ptr, float(conductivity), out))
        return np.array(out[:2 * self.dim], dtype=np.float64)

    def dpp_nodal_flux(self, p, k1: float, k2: float, beta: float, mu: float):
        """(r1, r2) = residual of the un-eliminated DPP operator on the mixed field p (2n values, field-major): an array
        for an array, a new device tensor for a device tensor (pph_dpp_nodal_flux / pph_dpp_nodal_flux_device)."""
        keep, ptr, dev = self._nodal_arg(p, 2 * self.n, "mixed field")
        if dev:
            r = self._device_out(2 * self.n)
            self._check(lib.pph_dpp_nodal_flux_device(self._h, float(k1), float(k2), float(beta), float(mu), ptr, _tptr(r)))
            self.torch_waits()
            return r
        r = np.empty(2 * self.n, dtype=np.float64)
        self._check(lib.pph_dpp_nodal_flux(self._h, float(k1), float(k2), float(beta), float(mu), ptr, _ptr(r)))
        return r

    # -- adjoint (pph_adjoint.hip): a NumPy array is uploaded for the call, a device tensor is read where it is ----
    def solve_rhs(self, cfg: SolverCfg, b, hist_cap: int = 0, raise_on_diverged: bool = True):
        """x with F A F x = F b for the assembled system (pph_solve_rhs / pph_solve_rhs_device): b a 2n array or device
        tensor, x of the same kind (0 on constrained dofs).  Returns (x, info, hist) as solve() does; the context's own
        right-hand side and solution are left as they were."""
        keep, ptr, dev = self._nodal_arg(b, 2 * self.n, "right-hand side")
        info = SolveInfo()
        hist = np.zeros(max(hist_cap, 1), dtype=np.float64)
        if dev:
            x = self._device_out(2 * self.n)
            st = lib.pph_solve_rhs_device(self._h, C.byref(cfg), ptr, _tptr(x), C.byref(info), _ptr(hist), int(hist_cap))
            self.torch_waits()
        else:
            x = np.empty(2 * self.n, dtype=np.float64)
            st = lib.pph_solve_rhs(self._h, C.byref(cfg), ptr, _ptr(x), C.byref(info), _ptr(hist), int(hist_cap))
        self.last_info = info
        self._check(st, allow_diverged=not raise_on_diverged)
        nh = min(hist_cap, info.iterations + 1)
        return x, info, hist[:nh].copy()

    def dpp_bilinear(self, lam, p) -> tuple:
        """(o0, o1, o2) = (lam1^T K p1, lam2^T K p2, (lam1 - lam2)^T M (p1 - p2)) of two mixed fields (2n values each,
        field-major; arrays or device tensors), in one matrix-free pass (pph_dpp_bilinear / pph_dpp_bilinear_device)."""
        keep_l, lptr, ldev = self._nodal_arg(lam, 2 * self.n, "adjoint field")
        keep_p, pptr, pdev = self._nodal_arg(p, 2 * self.n, "mixed field")
        if ldev != pdev:
            raise ValueError("dpp_bilinear: both fields must be arrays or both device tensors")
        out = (C.c_double * 3)()
        fn = lib.pph_dpp_bilinear_device if ldev else lib.pph_dpp_bilinear
        self._check(fn(self._h, lptr, pptr, out))
        return out[0], out[1], out[2]

    # -- transient (pph_transient.hip): a NumPy array is uploaded for the call, a device tensor is read where it is ----
    def step_rhs(self, p, k1: float, k2: float, beta: float, mu: float):
        """b = -F A_unel p, the right-hand side of a theta step in delta form, for the mixed field p (2n values,
        field-major): minus ``dpp_nodal_flux(p)`` with exact zeros on the dofs the Dirichlet sets constrain.  An array for
        an array, a new device tensor for a device tensor (pph_dpp_step_rhs / pph_dpp_step_rhs_device); matrix-free on
        degree-1 meshes."""
        keep, ptr, dev = self._nodal_arg(p, 2 * self.n, "mixed field")
        if dev:
            b = self._device_out(2 * self.n)
            self._check(lib.pph_dpp_step_rhs_device(self._h, float(k1), float(k2), float(beta), float(mu), ptr, _tptr(b)))
            self.torch_waits()
            return b
        b = np.empty(2 * self.n, dtype=np.float64)
        self._check(lib.pph_dpp_step_rhs(self._h, float(k1), float(k2), float(beta), float(mu), ptr, _ptr(b)))
        return b

    def transient_begin(self, k1: float, k2: float, beta: float, mu: float, storage, theta: float, dt: float,
                        monolithic: bool = True) -> None:
        """Assembles the operator Sigma M / dt + theta A of a theta step (storage = (S1, S2) > 0, 1/2 <= theta <= 1, dt > 0)
        and records the steady coefficients for ``transient_steps`` (pph_transient_begin)."""
        S1, S2 = (float(v) for v in storage)
        self._check(lib.pph_transient_begin(self._h, float(k1), float(k2), float(beta), float(mu), S1, S2, float(theta),
                                            float(dt), int(monolithic)))

    def transient_steps(self, cfg: SolverCfg, p, nsteps: int, steady_tol: float = 0.0, raise_on_diverged: bool = True,
                        record: bool = False, coef=None):
        """Advances the mixed field p (2n values, field-major) by up to `nsteps` theta steps IN PLACE: a float64 NumPy array
        (copied in and out) or a device tensor (pph_transient_steps / pph_transient_steps_device).  Returns (steps_done,
        infos [steps_done] of SolveInfo, norms [steps_done, 2] = (||b_s||, ||d_s||)); with ``record`` a fourth entry, the
        trajectory [steps_done + 1, 2n] of the same kind as p (pph_transient_steps_record*).  ``coef``: None, or the
        coefficient rows [nsteps, K] of the context's source set (``sources_set``): step s adds F sum_k coef[s, k] L_k to its
        right-hand side (pph_transient_steps_sources*)."""
        nsteps = int(nsteps)
        if coef is not None:
            return self._transient_steps_sources(cfg, p, nsteps, steady_tol, raise_on_diverged, record, coef)
        if record:
            return self._transient_steps_record(cfg, p, nsteps, steady_tol, raise_on_diverged)
        infos = (SolveInfo * max(nsteps, 1))()
        norms = np.zeros((max(nsteps, 1), 2), dtype=np.float64)
        done = C.c_int(0)
        if isinstance(p, np.ndarray):
            if p.dtype != np.float64 or p.shape != (2 * self.n,) or not p.flags.c_contiguous or not p.flags.writeable:
                raise ValueError(f"transient_steps: p must be a writeable contiguous float64 array of {2 * self.n} values")
            st = lib.pph_transient_steps(self._h, C.byref(cfg), _ptr(p), nsteps, float(steady_tol), infos, _ptr(norms),
                                         C.byref(done))
        else:
            t = self._device_in(p, 2 * self.n, "mixed field")
            if t.data_ptr() != p.data_ptr():
                raise ValueError("transient_steps: p must be a contiguous float64 device tensor (it is advanced in place)")
            st = lib.pph_transient_steps_device(self._h, C.byref(cfg), _tptr(t), nsteps, float(steady_tol), infos, _ptr(norms),
                                                C.byref(done))
            self.torch_waits()
        k = int(done.value)
        self.last_info = infos[k - 1] if k > 0 else SolveInfo()
        self._check(st, allow_diverged=not raise_on_diverged)
        return k, [infos[i] for i in range(k)], norms[:k].copy()

    def _transient_steps_record(self, cfg: SolverCfg, p, nsteps: int, steady_tol: float, raise_on_diverged: bool):
        infos = (SolveInfo * max(nsteps, 1))()
        norms = np.zeros((max(nsteps, 1), 2), dtype=np.float64)
        done = C.c_int(0)
        if isinstance(p, np.ndarray):
            if p.dtype != np.float64 or p.shape != (2 * self.n,) or not p.flags.c_contiguous or not p.flags.writeable:
                raise ValueError(f"transient_steps: p must be a writeable contiguous float64 array of {2 * self.n} values")
            traj = np.zeros((max(nsteps, 0) + 1, 2 * self.n), dtype=np.float64)
            st = lib.pph_transient_steps_record(self._h, C.byref(cfg), _ptr(p), nsteps, float(steady_tol), infos, _ptr(norms),
                                                C.byref(done), _ptr(traj))
        else:
            t = self._device_in(p, 2 * self.n, "mixed field")
            if t.data_ptr() != p.data_ptr():
                raise ValueError("transient_steps: p must be a contiguous float64 device tensor (it is advanced in place)")
            traj = self._device_out((max(nsteps, 0) + 1) * 2 * self.n).reshape(max(nsteps, 0) + 1, 2 * self.n)
            st = lib.pph_transient_steps_record_device(self._h, C.byref(cfg), _tptr(t), nsteps, float(steady_tol), infos,
                                                       _ptr(norms), C.byref(done), _tptr(traj))
            self.torch_waits()
        k = int(done.value)
        self.last_info = infos[k - 1] if k > 0 else SolveInfo()
        self._check(st, allow_diverged=not raise_on_diverged)
        return k, [infos[i] for i in range(k)], norms[:k].copy(), traj[:k + 1]

    def _transient_steps_sources(self, cfg: SolverCfg, p, nsteps: int, steady_tol: float, raise_on_diverged: bool, record: bool,
                                 coef):
        c = np.ascontiguousarray(coef, dtype=np.float64)
        if c.ndim != 2 or c.shape[0] != nsteps:
            raise ValueError(f"transient_steps: coef must have shape [{nsteps}, K], got {c.shape}")
        K = int(c.shape[1])
        infos = (SolveInfo * max(nsteps, 1))()
        norms = np.zeros((max(nsteps, 1), 2), dtype=np.float64)
        done = C.c_int(0)
        rows = max(nsteps, 0) + 1
        traj = None
        if isinstance(p, np.ndarray):
            if p.dtype != np.float64 or p.shape != (2 * self.n,) or not p.flags.c_contiguous or not p.flags.writeable:
                raise ValueError(f"transient_steps: p must be a writeable contiguous float64 array of {2 * self.n} values")
            if record:
                traj = np.zeros((rows, 2 * self.n), dtype=np.float64)
            st = lib.pph_transient_steps_sources(self._h, C.byref(cfg), _ptr(p), nsteps, float(steady_tol), infos, _ptr(norms),
                                                 C.byref(done), _ptr(traj), _ptr(c), K)
        else:
            t = self._device_in(p, 2 * self.n, "mixed field")
            if t.data_ptr() != p.data_ptr():
                raise ValueError("transient_steps: p must be a contiguous float64 device tensor (it is advanced in place)")
            if record:
                traj = self._device_out(rows * 2 * self.n).reshape(rows, 2 * self.n)
            st = lib.pph_transient_steps_sources_device(self._h, C.byref(cfg), _tptr(t), nsteps, float(steady_tol), infos,
                                                        _ptr(norms), C.byref(done), None if traj is None else _tptr(traj),
                                                        _ptr(c), K)
            self.torch_waits()
        k = int(done.value)
        self.last_info = infos[k - 1] if k > 0 else SolveInfo()
        self._check(st, allow_diverged=not raise_on_diverged)
        out = (k, [infos[i] for i in range(k)], norms[:k].copy())
        return out + (traj[:k + 1],) if record else out

    # -- sources of the transient runs (pph_sources.hip) ------------------------------------------------------------------
    def sources_set(self, dense=None, points=None, fields=None, tol: float = 1e-12) -> int:
        """Replaces the context's source set (pph_sources_set*): ``dense`` [n_dense, 2n] load vectors (or None), ``points``
        [m, dim] with the network ``fields`` [m] (0 or 1) of every point (or None).  Arrays, or device tensors for dense and
        points (both of one kind).  Source k < n_dense is dense load k, source n_dense + p point p.  Returns the number of
        points outside the mesh (they keep their place in the numbering and load nothing)."""
        dev = (dense is not None and not isinstance(dense, np.ndarray)) or (points is not None and not isinstance(points, np.ndarray))
        nd = 0 if dense is None else int(dense.shape[0])
        m = 0 if points is None else int(points.shape[0])
        if dense is not None and tuple(dense.shape) != (nd, 2 * self.n):
            raise ValueError(f"sources_set: dense must have shape [n_dense, {2 * self.n}], got {tuple(dense.shape)}")
        if points is not None and (len(points.shape) != 2 or points.shape[1] != self.dim):
            raise ValueError(f"sources_set: points must have shape [m, {self.dim}], got {tuple(points.shape)}")
        fld = np.zeros(m, dtype=np.int32) if fields is None else np.ascontiguousarray(fields, dtype=np.int32).reshape(-1)
        if fld.shape != (m,):
            raise ValueError(f"sources_set: fields must hold one network index per point ({m}), got {fld.shape}")
        nout = C.c_int64()
        if dev:
            if (dense is not None and isinstance(dense, np.ndarray)) or (points is not None and isinstance(points, np.ndarray)):
                raise ValueError("sources_set: dense and points must be arrays or both device tensors")
            d = None if nd == 0 else self._device_in(dense.reshape(-1), nd * 2 * self.n, "dense")
            x = None if m == 0 else self._device_in(points.reshape(-1), m * self.dim, "points")
            self._check(lib.pph_sources_set_device(self._h, None if d is None else _tptr(d), nd, None if x is None else _tptr(x),
                                                   _ptr(fld), m, float(tol), C.byref(nout)))
        else:
            d = None if nd == 0 else np.ascontiguousarray(dense, dtype=np.float64)
            x = None if m == 0 else np.ascontiguousarray(points, dtype=np.float64)
            self._check(lib.pph_sources_set(self._h, _ptr(d), nd, _ptr(x), _ptr(fld), m, float(tol), C.byref(nout)))
        return int(nout.value)

    def sources_clear(self) -> None:
        self._check(lib.pph_sources_clear(self._h))

    def sources_count(self) -> int:
        """Number of sources K of the context's set, -1 without one (pph_sources_count)."""
        k = C.c_int64()
        self._check(lib.pph_sources_count(self._h, C.byref(k)))
        return int(k.value)

    def sources_apply(self, coef, b):
        """b += F sum_k coef[k] L_k IN PLACE for one coefficient row coef [K]; b: 2n values, a writeable float64 array or a
        device tensor (pph_sources_apply / pph_sources_apply_device).  Returns b."""
        c = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
        K = self.sources_count()
        if K >= 0 and c.shape != (K,):
            raise ValueError(f"sources_apply: coef must hold {K} values, got {c.shape}")
        if isinstance(b, np.ndarray):
            if b.dtype != np.float64 or b.shape != (2 * self.n,) or not b.flags.c_contiguous or not b.flags.writeable:
                raise ValueError(f"sources_apply: b must be a writeable contiguous float64 array of {2 * self.n} values")
            self._check(lib.pph_sources_apply(self._h, _ptr(c), _ptr(b)))
            return b
        t = self._device_in(b, 2 * self.n, "right-hand side")
        if t.data_ptr() != b.data_ptr():
            raise ValueError("sources_apply: b must be a contiguous float64 device tensor (it is added to in place)")
        self._check(lib.pph_sources_apply_device(self._h, _ptr(c), _tptr(t)))
        self.torch_waits()
        return b

    # -- transient adjoint (pph_transient_adjoint.hip) ------------------------------------------------------------------
    def transient_bilinear(self, w, p0, p1, theta: float) -> tuple:
        """The five forms of one backward step, (w1^T K pm1, w2^T K pm2, (w1 - w2)^T M (pm1 - pm2), w1^T M d1, w2^T M d2) with
        pm = p0 + theta (p1 - p0), d = p1 - p0, of three mixed fields (2n values each; all arrays or all device tensors), in
        one matrix-free pass (pph_transient_bilinear / pph_transient_bilinear_device)."""
        args = [self._nodal_arg(v, 2 * self.n, name) for v, name in ((w, "adjoint field"), (p0, "state"), (p1, "next state"))]
        if len({a[2] for a in args}) != 1:
            raise ValueError("transient_bilinear: the three fields must be arrays or all device tensors")
        out = (C.c_double * 5)()
        fn = lib.pph_transient_bilinear_device if args[0][2] else lib.pph_transient_bilinear
        self._check(fn(self._h, args[0][1], args[1][1], args[2][1], float(theta), out))
        return tuple(out[i] for i in range(5))

    def eval_points_adjoint(self, points, weights, out=None, ncomp: int = 1, tol: float = 1e-12):
        """The transpose of eval_points: (out [n * ncomp] with out[node, k] += sum_m phi_node(x_m) weights[m, k], number of
        points outside).  points [m, dim], weights [m, ncomp]: arrays or device tensors (pph_eval_points_adjoint*); ``out``
        is added to IN PLACE when given (same kind), else starts from zeros.  Points are taken one after the other: linear
        in m."""
        ncomp = int(ncomp)
        nout = C.c_int64()
        if isinstance(points, np.ndarray):
            x = np.ascontiguousarray(points, dtype=np.float64)
            c = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1, ncomp)
            if x.ndim != 2 or x.shape[1] != self.dim or c.shape[0] != x.shape[0]:
                raise ValueError(f"points must be [m, {self.dim}] and weights [m, {ncomp}], got {x.shape}, {c.shape}")
            if out is None:
                out = np.zeros(self.n * ncomp, dtype=np.float64)
            elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (self.n * ncomp,)
                      and out.flags.c_contiguous and out.flags.writeable):
                raise ValueError(f"out must be a writeable contiguous float64 array of {self.n * ncomp} values")
            self._check(lib.pph_eval_points_adjoint(self._h, _ptr(x), int(x.shape[0]), _ptr(c), ncomp, float(tol), _ptr(out),
                                                    C.byref(nout)))
            return out, int(nout.value)
        import torch

        if not (isinstance(points, torch.Tensor) and points.dtype == torch.float64 and points.is_cuda and points.dim() == 2
                and points.shape[1] == self.dim and points.is_contiguous() and points.device.index == self.device):
            raise ValueError(f"points must be a contiguous float64 tensor [m, {self.dim}] on cuda:{self.device}")
        m = points.shape[0]
        c = self._device_in(weights.reshape(-1), m * ncomp, "weights")
        if out is None:
            out = torch.zeros(self.n * ncomp, dtype=torch.float64, device=self.torch_device())
        else:
            o = self._device_in(out, self.n * ncomp, "out")
            if o.data_ptr() != out.data_ptr():
                raise ValueError("out must be a contiguous float64 device tensor (it is added to in place)")
        self.wait_for_torch()
        self._check(lib.pph_eval_points_adjoint_device(self._h, _tptr(points), int(m), _tptr(c), ncomp, float(tol), _tptr(out),
                                                       C.byref(nout)))
        self.torch_waits()
        return out, int(nout.value)

    def transient_adjoint(self, cfg: SolverCfg, traj, g=None, obs_x=None, obs_c=None, obs_tol: float = 1e-12,
                          want_wsum: bool = True, raise_on_diverged: bool = True, want_src_grad: bool = False):
        """The backward loop over a recorded trajectory traj [N + 1, 2n] (pph_transient_adjoint*): g [N + 1, 2n] and / or the
        observation form obs_x [m, dim], obs_c [N + 1, m, 2]; all arrays or all device tensors.  Returns (terms [N, 5] array,
        q0, wsum or None, infos [steps_done], steps_done); q0 and wsum are of the kind of traj.  ``want_src_grad``: a sixth
        entry, src_grad [N, K] array with src_grad[s, k] = w_s^T F L_k for the K sources of the context's set
        (pph_transient_adjoint_sources*)."""
        dev = not isinstance(traj, np.ndarray)
        n2 = 2 * self.n
        if tuple(traj.shape[1:]) != (n2,) or traj.shape[0] < 2:
            raise ValueError(f"traj must have shape [N + 1, {n2}] with N >= 1, got {tuple(traj.shape)}")
        N = int(traj.shape[0]) - 1
        if g is None and obs_c is None:
            raise ValueError("transient_adjoint: neither g nor the observation form is given")
        if (obs_c is None) != (obs_x is None):
            raise ValueError("transient_adjoint: obs_x and obs_c go together")
        m = 0 if obs_x is None else int(obs_x.shape[0])
        if g is not None and tuple(g.shape) != (N + 1, n2):
            raise ValueError(f"g must have shape [{N + 1}, {n2}], got {tuple(g.shape)}")
        if obs_c is not None and (tuple(obs_x.shape) != (m, self.dim) or tuple(obs_c.shape) != (N + 1, m, 2)):
            raise ValueError(f"obs_x must be [m, {self.dim}] and obs_c [{N + 1}, m, 2], got {tuple(obs_x.shape)}, "
                             f"{tuple(obs_c.shape)}")
        terms = np.zeros((N, 5), dtype=np.float64)
        infos = (SolveInfo * N)()
        done = C.c_int(0)
        sg, extra = None, ()
        if want_src_grad:
            K = self.sources_count()
            if K < 0:
                raise ValueError("transient_adjoint: the context holds no source set (sources_set)")
            sg = np.zeros((N, K), dtype=np.float64)
            extra = (_ptr(sg), K)
        if dev:
            flat = lambda v, cnt, name: None if v is None else self._device_in(v.reshape(-1), cnt, name)
            tj, gg = flat(traj, (N + 1) * n2, "traj"), flat(g, (N + 1) * n2, "g")
            ox, oc = flat(obs_x, m * self.dim, "obs_x"), flat(obs_c, (N + 1) * m * 2, "obs_c")
            q0 = self._device_out(n2)
            wsum = self._device_out(n2) if want_wsum else None
            fn = lib.pph_transient_adjoint_sources_device if want_src_grad else lib.pph_transient_adjoint_device
            st = fn(self._h, C.byref(cfg), _tptr(tj), None if gg is None else _tptr(gg), None if ox is None else _tptr(ox), m,
                    None if oc is None else _tptr(oc), float(obs_tol), N, _ptr(terms), _tptr(q0),
                    None if wsum is None else _tptr(wsum), infos, C.byref(done), *extra)
            self.torch_waits()
        else:
            arr = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
            tj, gg, ox, oc = arr(traj), arr(g), arr(obs_x), arr(obs_c)
            q0 = np.zeros(n2, dtype=np.float64)
            wsum = np.zeros(n2, dtype=np.float64) if want_wsum else None
            fn = lib.pph_transient_adjoint_sources if want_src_grad else lib.pph_transient_adjoint
            st = fn(self._h, C.byref(cfg), _ptr(tj), _ptr(gg), _ptr(ox), m, _ptr(oc), float(obs_tol), N, _ptr(terms), _ptr(q0),
                    _ptr(wsum), infos, C.byref(done), *extra)
        k = int(done.value)
        self.last_info = infos[N - k] if k > 0 else SolveInfo()
        self._check(st, allow_diverged=not raise_on_diverged)
        out = (terms, q0, wsum, [infos[s] for s in range(N - k, N)], k)
        return out + (sg,) if want_src_grad else out

    # -- export -------------------------------------------------------------------------------
    def csr(self, which: int):
        import scipy.sparse as sp

        nrows, nnz = C.c_int64(), C.c_int64()
        self._check(lib.pph_csr_sizes(self._h, which, C.byref(nrows), C.byref(nnz)))
        rowptr = np.empty(nrows.value + 1, dtype=np.int64)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value, dtype=np.float64)
        self._check(lib.pph_get_csr(self._h, which, _ptr(rowptr), _ptr(col), _ptr(val)))
        return sp.csr_matrix((val, col, rowptr), shape=(nrows.value, nrows.value))

    def rhs(self):
        r = np.empty(2 * self.n, dtype=np.float64)
        u0 = np.empty(2 * self.n, dtype=np.float64)
        self._check(lib.pph_get_rhs(self._h, _ptr(r), _ptr(u0)))
        return r, u0

    def spmv(self, which: int, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        self._check(lib.pph_spmv(self._h, which, _ptr(x), _ptr(y)))
        return y

    def pc_apply(self, which: int, pc_type: int, r: np.ndarray, mg_smooth: int = 2) -> np.ndarray:
        """z = B r: one application of the block preconditioner `pc_type` (PC_JACOBI, PC_MG, PC_PMG, PC_ILU) of block
        `which` (0: A11, 1: A22) of the assembled system.  Entries of r on constrained dofs count as 0."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.shape != (self.n,):
            raise ValueError(f"pc_apply: r must have shape ({self.n},)")
        z = np.empty_like(r)
        self._check(lib.pph_pc_apply(self._h, int(which), int(pc_type), int(mg_smooth), _ptr(r), _ptr(z)))
        return z

    def pc_apply_coupled(self, pc_type: int, r: np.ndarray, mg_smooth: int = 2) -> np.ndarray:
        """z = B r: one application of the monolithic preconditioner `pc_type` (PC_CMG, PC_BLOCK2, PC_JACOBI) to a
        field-major vector of 2n entries (needs the monolithic assembly).  Entries of r on constrained dofs count as 0."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.shape != (2 * self.n,):
            raise ValueError(f"pc_apply_coupled: r must have shape ({2 * self.n},)")
        z = np.empty_like(r)
        self._check(lib.pph_pc_apply_coupled(self._h, int(pc_type), int(mg_smooth), _ptr(r), _ptr(z)))
        return z

    def cmg_bench(self, reps: int, mg_smooth: int = 2) -> dict:
        """Timing of `reps` coupled cycles and of the fine-level coupled smoothing kernel alone (tools/cmg_probe.py)."""
        out = np.zeros(4, dtype=np.float64)
        self._check(lib.pph_cmg_bench(self._h, int(mg_smooth), int(reps), out.ctypes.data_as(C.POINTER(C.c_double))))
        return {"cycle_ms": out[0], "step_ms": out[1], "step_bytes": out[2], "setup_ms": out[3]}

    def pc_bench(self, which: int, pc_type: int, reps: int, mg_smooth: int = 2) -> dict:
        """Timing of `reps` applications of a block preconditioner on the device (tools/pmg_probe.py)."""
        out = np.zeros(4, dtype=np.float64)
        self._check(lib.pph_pc_bench(self._h, int(which), int(pc_type), int(mg_smooth), int(reps),
                                     out.ctypes.data_as(C.POINTER(C.c_double))))
        return {"apply_ms": out[0], "level0_ms": out[1], "level0_bytes": out[2], "setup_ms": out[3]}

    def extreme_eigenvalues(self, which: int, tol: float = 1e-10, max_it: int = 20000, check_every: int = 32,
                            vectors: bool = False) -> dict:
        """lambda_min and lambda_max of a symmetric operator of the context (MAT_MONO, MAT_M, MAT_A11, MAT_A22) by plain
        Lanczos on the device (pph_extreme_eigenvalues): nothing but the recurrence coefficients reaches the host.  Returns
        the fields of its `out`; `converged` 0 means stopped at max_it (values still returned).  vectors=True: also the two
        normalised Ritz vectors as device tensors (`vector_min`, `vector_max`), their Rayleigh quotients and true residual
        norms ||A y - rq y||."""
        out = np.zeros(13, dtype=np.float64)
        ylo = yhi = None
        if vectors:
            require_shared_runtime("extreme_eigenvalues(vectors=True)")
            nrows = 2 * self.n if int(which) == MAT_MONO else self.n
            ylo, yhi = self._device_out(nrows), self._device_out(nrows)
        self._check(lib.pph_extreme_eigenvalues(self._h, int(which), float(tol), int(max_it), int(check_every),
                                                _tptr(ylo) if vectors else None, _tptr(yhi) if vectors else None,
                                                out.ctypes.data_as(C.POINTER(C.c_double))))
        res = {"lambda_min": float(out[0]), "lambda_max": float(out[1]), "iterations": int(out[2]), "converged": int(out[3]),
               "breakdown": int(out[4]), "estimate_min": float(out[5]), "estimate_max": float(out[6]),
               "device_ms": float(out[7]), "krylov_dimension": int(out[12])}
        if vectors:
            self.torch_waits()
            res.update(vector_min=ylo, vector_max=yhi, rayleigh_min=float(out[8]), rayleigh_max=float(out[9]),
                       residual_min=float(out[10]), residual_max=float(out[11]))
        return res

    def preconditioned_extremes(self, which: int, pc_type: int, mg_smooth: int = 2, tol: float = 1e-4, max_it: int = 2000,
                                check_every: int = 16) -> dict:
        """lambda_min and lambda_max of B A on the free rows - A the operator `which` (MAT_MONO, MAT_M, MAT_A11, MAT_A22), B
        the symmetric preconditioner `pc_type` (blocks: PC_JACOBI, PC_ILU, PC_MG, PC_PMG; monolithic: PC_JACOBI, PC_BLOCK2,
        PC_ILU, PC_CMG; M: PC_JACOBI) - by Lanczos in the B inner product on the device (pph_preconditioned_extremes).  Returns the
        keys of extreme_eigenvalues plus `setup_ms` (the preconditioner's set-up, 0 when it was up to date) and `kappa` =
        lambda_max / lambda_min (inf when lambda_min is not positive); `converged` 0 means stopped at max_it."""
        out = np.zeros(10, dtype=np.float64)
        self._check(lib.pph_preconditioned_extremes(self._h, int(which), int(pc_type), int(mg_smooth), float(tol), int(max_it),
                                                    int(check_every), out.ctypes.data_as(C.POINTER(C.c_double))))
        lo, hi = float(out[0]), float(out[1])
        return {"lambda_min": lo, "lambda_max": hi, "iterations": int(out[2]), "converged": int(out[3]),
                "breakdown": int(out[4]), "estimate_min": float(out[5]), "estimate_max": float(out[6]),
                "device_ms": float(out[7]), "krylov_dimension": int(out[8]), "setup_ms": float(out[9]),
                "kappa": hi / lo if lo > 0.0 else float("inf")}

    def spmv_bench(self, which: int, reps: int) -> float:
        ms = C.c_double()
        self._check(lib.pph_spmv_bench(self._h, which, int(reps), C.byref(ms)))
        return ms.value

    def error_norms_mms(self, field: int, nodal: np.ndarray, k1: float, k2: float, beta: float, mu: float, nq: int = 6):
        """(L2 error, H1-seminorm error) of a nodal CG-1 field against the manufactured pressure `field`."""
        nodal = np.ascontiguousarray(nodal, dtype=np.float64)
        if nodal.shape != (self.n,):
            raise ValueError("nodal array must have one value per mesh vertex")
        l2, h1 = C.c_double(), C.c_double()
        self._check(lib.pph_error_norms_mms(self._h, int(field), _ptr(nodal), float(k1), float(k2), float(beta), float(mu),
                                            int(nq), C.byref(l2), C.byref(h1)))
        return l2.value, h1.value

    def eval_points(self, nodal: np.ndarray, points: np.ndarray, ncomp: int = 1, gradient: bool = False, tol: float = 1e-12):
        """Values of the field nodal [n * ncomp] (node-major) at points [m, dim] (pph_eval_points): (values [m, ncomp],
        gradients [m, ncomp, dim] or None, number of outside points - whose rows are NaN)."""
        nodal = np.ascontiguousarray(nodal, dtype=np.float64).reshape(-1)
        points = np.ascontiguousarray(points, dtype=np.float64)
        if nodal.shape != (self.n * int(ncomp),):
            raise ValueError(f"expected {self.n * int(ncomp)} nodal values, got {nodal.shape}")
        if points.ndim != 2 or points.shape[1] != self.dim:
            raise ValueError(f"points must have shape [m, {self.dim}], got {points.shape}")
        m = points.shape[0]
        val = np.empty((m, int(ncomp)), dtype=np.float64)
        grad = np.empty((m, int(ncomp), self.dim), dtype=np.float64) if gradient else None
        nout = C.c_int64()
        self._check(lib.pph_eval_points(self._h, _ptr(nodal), int(ncomp), _ptr(points), int(m), float(tol), _ptr(val),
                                        _ptr(grad), C.byref(nout)))
        return val, grad, int(nout.value)

    def trace_pathlines(self, nodal: np.ndarray, seeds: np.ndarray, scale: float, dt: float, max_steps: int,
                        min_speed: float = 0.0, chunk: int = 4096, record_every: int = 0):
        """Pathlines of v = scale * u_h, u_h the CG-1 vector field nodal [n * dim] (node-major), from seeds [m, dim]
        (pph_trace_pathlines): (end [m, dim], time [m], length [m], steps [m] int32, status [m] int32 (status | side << 8),
        path [n_rec, m, dim] or None, counts [4])."""
        nodal = np.ascontiguousarray(nodal, dtype=np.float64).reshape(-1)
        seeds = np.ascontiguousarray(seeds, dtype=np.float64)
        if nodal.shape != (self.n * self.dim,):
            raise ValueError(f"expected {self.n * self.dim} nodal values, got {nodal.shape}")
        if seeds.ndim != 2 or seeds.shape[1] != self.dim:
            raise ValueError(f"seeds must have shape [m, {self.dim}], got {seeds.shape}")
        m = seeds.shape[0]
        n_rec = int(max_steps) // int(record_every) + 1 if record_every > 0 else 0
        end = np.empty((m, self.dim), dtype=np.float64)
        time, length = np.empty(m, dtype=np.float64), np.empty(m, dtype=np.float64)
        steps, status = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int32)
        path = np.empty((n_rec, m, self.dim), dtype=np.float64) if n_rec else None
        counts = (C.c_int64 * 4)()
        self._check(lib.pph_trace_pathlines(self._h, _ptr(nodal), float(scale), _ptr(seeds), int(m), float(dt), int(max_steps),
                                            float(min_speed), int(chunk), int(record_every), _ptr(end), _ptr(time), _ptr(length),
                                            _ptr(steps), _ptr(status), _ptr(path), counts))
        return end, time, length, steps, status, path, list(counts)

    def quadrature_points(self, nq: int, cell_begin: int, cell_count: int) -> np.ndarray:
        """Physical coordinates [cell_count * nq**dim, dim] of the Gauss points of a cell range (pph_quadrature_points)."""
        npts = nq ** self.dim
        out = np.empty((cell_count * npts, self.dim), dtype=np.float64)
        self._check(lib.pph_quadrature_points(self._h, int(nq), int(cell_begin), int(cell_count), _ptr(out)))
        return out

    def error_norms_sampled(self, nodal: np.ndarray, exact, grad=None, nq: int = 6, chunk_cells: int = 1 << 16):
        """(L2 error, H1-seminorm error) of a nodal CG-1 field against `exact`, a callable of point arrays [m, dim] -> [m]
        (None: the zero field), with `grad` its gradient callable [m, dim] -> [m, dim] (None: central differences of
        `exact` with step 1e-6).  The cells are processed in chunks: points out, samples in."""
        nodal = np.ascontiguousarray(nodal, dtype=np.float64)
        if nodal.shape != (self.n,):
            raise ValueError("nodal array must have one value per mesh vertex")
        l2, h1 = 0.0, 0.0
        a, b = C.c_double(), C.c_double()
        if exact is None:
            chunk_cells = self.ncell      # no host samples: one call over all cells
        first = True
        for c0 in range(0, self.ncell, chunk_cells):
            cnt = min(chunk_cells, self.ncell - c0)
            se = sg = None
            if exact is not None:
                se, sg = self._samples(exact, grad, nq, c0, cnt)
            # the nodal field travels with the first chunk only (NULL afterwards = the field of the previous call)
            self._check(lib.pph_error_norms_sampled(self._h, _ptr(nodal) if first else None, int(nq), int(c0), int(cnt),
                                                    _ptr(se), _ptr(sg), C.byref(a), C.byref(b)))
            first = False
            l2 += a.value
            h1 += b.value
        return float(np.sqrt(l2)), float(np.sqrt(h1))

    def _samples(self, exact, grad, nq: int, c0: int, cnt: int):
        """Exact field and gradient at the quadrature points of cells [c0, c0 + cnt) (host arrays)."""
        X = self.quadrature_points(nq, c0, cnt)
        se = np.ascontiguousarray(exact(X), dtype=np.float64).reshape(-1)
        if grad is not None:
            sg = np.ascontiguousarray(grad(X), dtype=np.float64).reshape(-1, self.dim)
        else:
            h = 1e-6
            sg = np.empty_like(X)
            for d in range(self.dim):
                E = np.zeros(self.dim)
                E[d] = h
                sg[:, d] = (np.asarray(exact(X + E), dtype=np.float64).reshape(-1)
                            - np.asarray(exact(X - E), dtype=np.float64).reshape(-1)) / (2 * h)
            sg = np.ascontiguousarray(sg)
        return se, sg

    def darcy_velocity(self, nodal: np.ndarray, conductivity: float) -> np.ndarray:
        """L2 projection of -conductivity * grad(p_h) onto CG-1 vectors; returns [n, dim]."""
        nodal = np.ascontiguousarray(nodal, dtype=np.float64)
        if nodal.shape != (self.n,):
            raise ValueError("nodal array must have one value per mesh vertex")
        out = np.empty((self.n, self.dim), dtype=np.float64)
        self._check(lib.pph_darcy_velocity(self._h, _ptr(nodal), float(conductivity), _ptr(out)))
        return out

    def comm_stats(self) -> dict:
        h, a, st = C.c_int64(), C.c_int64(), C.c_int()
        self._check(lib.pph_comm_stats(self._h, C.byref(h), C.byref(a), C.byref(st)))
        return {"halo_exchanges": h.value, "allreduces": a.value, "status": st.value}

    def comm_times(self) -> dict:
        """Summed durations of the last solve's exchanges / reductions (option time_comm)."""
        t = (C.c_double * 4)()
        self._check(lib.pph_comm_times(self._h, t))
        return {"halo_ms": t[0], "allreduce_ms": t[1], "halo_timed": int(t[2]), "allreduce_timed": int(t[3])}

    def timers(self) -> dict:
        t = np.zeros(36 + 1, dtype=np.float64)     # (out[0..35], and out[36] of option l3_order)
        self._check(lib.pph_get_timers(self._h, _ptr(t), t.size))
        return {"mesh_ms": t[0], "assemble_ms": t[1], "bc_blocks_ms": t[2], "solve_ms": t[3],
                "spmv_ms": t[4], "spmv_launches": int(t[5]), "spmv_bytes": t[6],
                "spmv_dot_ms": t[7], "spmv_dot_launches": int(t[8]), "spmv_dot_bytes": t[9],
                "halo_exchanges": int(t[10]),
                "spmv_fine_ms": t[11], "spmv_fine_launches": int(t[12]), "spmv_fine_bytes": t[13],
                "split_products": int(t[14]), "symmetric_storage": bool(t[15]),
                "max_split_partials": int(t[16]),
                "dict_operators": int(t[17]), "dict_classes": int(t[18]), "dict_status": int(t[19]),
                "dict_build_ms": t[20], "dict_builds": int(t[21]), "dict_zconst": bool(t[22]),
                # rows the two launches of the fine level's node assembly stored last (0: one launch), rows of the level
                "asm_rows_straight": int(t[23]), "asm_rows_general": int(t[24]), "asm_rows": int(t[25]),
                # on-chip LU-equivalent block solves of the last solve: how many ran, how many ended short of their tolerance
                # (iteration limit or p.Ap <= 0; any of them sets SolveInfo.inner_failed), their CG iterations summed
                "onchip_solves": int(t[26]), "onchip_unconverged": int(t[27]), "onchip_cg_iterations": int(t[28]),
                # CG updates of the last solve launched without the next cycle's first guess (option presmooth_lazy), cycles
                # that then formed it themselves, updates that wrote one no cycle read
                "presmooth_skipped": int(t[29]), "presmooth_late": int(t[30]), "presmooth_unused": int(t[31]),
                # operator values on demand (option asm_store_values 0): the fine level's straight-line rows were not stored by
                # the last assembly; launches that wrote such rows when a reader asked (since the context was created); levels
                # whose dictionary was refused on the device while their values were left out (the repair launch wrote them)
                "asm_values_stale": int(t[32]), "asm_values_materialized": int(t[33]), "asm_store_repairs": int(t[34]),
                # product launches of the last solve / preconditioner application whose smoothing epilogue took 1 / a_ii from
                # a row dictionary's table of inverse diagonals instead of the dinv array (option sell_dict_dinv)
                "dict_dinv_products": int(t[35]),
                # fine-level launches of the last solve / preconditioner application that swept their vectors descending
                # (option l3_order; launches recorded into a replayed graph count once, at the capture)
                "l3_order_descending": int(t[36])}
