"""
``solve_dpp`` / ``solve_dpp_nonlinear`` / ``Solution`` — mirror of reference
``src/perphil/solvers/solver.py:14-128`` over the HIP library (no Firedrake/PETSc, no CPU fallback).

Same call surface: ``solve_dpp(W, model_params, bcs, solver_parameters={}, options_prefix="dpp")``
returns ``Solution(solution, iteration_number, residual_error)``; ``ValueError`` unless ``W`` is a
2-field mixed space (solver.py:61-62).  PETSc options are translated by ``translate_options``:

=====================================  =============================================================
reference option                        MI355X path
=====================================  =============================================================
ksp_type gmres | cg                     GMRES(30), classical Gram-Schmidt / CG on the monolithic CSR
pc_type none | jacobi                   same
pc_type fieldsplit (multiplicative)     same; block solves = inner CG with multigrid or Jacobi PC
ksp_type preonly + pc_type lu (MUMPS)   "direct-equivalent": field-split GMRES with multigrid-CG
                                        block solves run to 1e-13 relative residual; reports
                                        iteration_number 1 and residual 0.0 like PETSc's preonly
                                        (blocks of <= 4096 rows: one on-chip Jacobi-CG per block solve;
                                        one that ends short of 1e-12 sets info["inner_failed"] and warns)
pc_type ilu (pc_factor_levels 0)        ILU(0) in the natural row order, factorisation and triangular solves
                                        level-scheduled on the device (levels i + 2j + 4k of the lexicographic
                                        numbering), monolithic system or field-split / Picard blocks;
                                        block ksp_type gmres = restarted GMRES(30) on the block
pc_type pph_cmg                         coupled multigrid on the monolithic system (ksp_type cg | gmres | preonly): one
                                        symmetric V-cycle over the CG-1 hierarchy whose Chebyshev smoother inverts the
                                        2 x 2 block of the two pressures of every node; pph_mg_smooth steps per level
                                        side (default 2).  Degree 1, one device; not a fieldsplit block pc
snes_type ngs | nrichardson             block Picard (fixed-stress) sweeps per dpp_delayed_form
                                        (dpp.py:196-203); the reference's PETSc secant-NGS history is
                                        not reproduced, the fixed point is
=====================================  =============================================================
"""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional, Tuple

import attr
import numpy as np

from . import _ffi, fd
from .forms import dpp_form, dpp_splitted_form
from .parameters import DPPParameters

_DIRECT_RTOL = 1e-13


@attr.define(frozen=True)
class Solution:
    """Result of a solve (reference solver.py:14-27) + ``info`` with what actually ran.  On a distributed mesh
    ``solution`` holds this rank's slab (``solution.owned()``: its owned rows); ``gather()`` returns the same result
    with the whole function on every rank.  ``solution`` is device-resident (``fd.Function.on_device``) when torch
    shares the library's HIP runtime: its values reach the host on first host access only."""
    solution: fd.Function | Tuple[fd.Function, fd.Function]
    iteration_number: int
    residual_error: float | np.float64
    info: dict = attr.field(factory=dict, eq=False)

    def gather(self) -> "Solution":
        sol = self.solution
        g = tuple(f.gather() for f in sol) if isinstance(sol, tuple) else sol.gather()
        return Solution(g, self.iteration_number, self.residual_error, self.info)


def _sub_options(params: Dict, idx: int) -> Dict:
    """Options of block `idx`: nested dict ``fieldsplit_i`` and/or flattened ``fieldsplit_i_*`` keys."""
    out = dict(params.get(f"fieldsplit_{idx}", {}) or {})
    pre = f"fieldsplit_{idx}_"
    for k, v in params.items():
        if isinstance(k, str) and k.startswith(pre):
            out[k[len(pre):]] = v
    return out


def _inner_cfg(cfg: _ffi.SolverCfg, subs: List[Dict], notes: List[str]) -> None:
    """Block-solve settings from the fieldsplit sub-options (both blocks share one setting)."""
    ksp = {s.get("ksp_type", "preonly") for s in subs}
    pc = {s.get("pc_type", "lu") for s in subs}
    rtols = [float(s["ksp_rtol"]) for s in subs if "ksp_rtol" in s]
    atols = [float(s["ksp_atol"]) for s in subs if "ksp_atol" in s]
    maxits = [int(s["ksp_max_it"]) for s in subs if "ksp_max_it" in s]
    k = ksp.pop() if len(ksp) == 1 else "cg"
    p = pc.pop() if len(pc) == 1 else "mg"
    cfg.inner_ksp_type = _ffi.KSP_CG
    cfg.inner_max_it = min(maxits) if maxits else 50000
    cfg.inner_atol = min(atols) if atols else 1e-50
    if p in ("lu", "cholesky"):
        # exact block solve of the reference -> multigrid-CG to a tight tolerance
        cfg.inner_pc_type, cfg.inner_rtol = _ffi.PC_MG, 1e-12
        cfg.inner_exact = 1      # (blocks of at most 4096 rows: one on-chip solve per block instead of a host-driven loop)
        notes.append("block LU -> CG + geometric multigrid, rtol 1e-12 (blocks of <= 4096 rows: one on-chip Jacobi-CG solve)")
        return
    if p == "pph_cmg":
        raise NotImplementedError("pc_type 'pph_cmg' is a cycle on the coupled system, not a fieldsplit block pc: use it as the "
                                  "top-level pc_type of a cg / gmres solve")
    if p not in ("mg", "pph_pmg", "jacobi", "none", "ilu"):
        raise NotImplementedError(f"fieldsplit block pc_type {p!r} is not supported (lu, ilu, mg, pph_pmg, jacobi, none)")
    # pph_pmg: the space's own operator on top of the CG-1 multigrid hierarchy of the same cells (degree 2; at degree 1 it is mg)
    cfg.inner_pc_type = {"mg": _ffi.PC_MG, "pph_pmg": _ffi.PC_PMG, "jacobi": _ffi.PC_JACOBI, "none": _ffi.PC_NONE,
                         "ilu": _ffi.PC_ILU}[p]
    if k == "preonly":
        cfg.inner_ksp_type = _ffi.KSP_PREONLY
    elif k in ("gmres", "fgmres"):
        cfg.inner_ksp_type = _ffi.KSP_GMRES      # restarted GMRES(30) on the block, as stated
    elif k == "cg":
        cfg.inner_ksp_type = _ffi.KSP_CG
    else:
        raise NotImplementedError(f"fieldsplit block ksp_type {k!r} is not supported")
    cfg.inner_rtol = min(rtols) if rtols else 1e-5  # PETSc default ksp_rtol
    # inexact block solves: ksp_norm_type of the sub-solvers (PETSc's option name) and the residual reduction each
    # block solve has to reach from its own starting residual (pph_reduction; 0 = ksp_rtol only)
    norms = {str(s.get("ksp_norm_type", "preconditioned")).lower() for s in subs}
    if len(norms) != 1 or norms - {"preconditioned", "unpreconditioned", "none"}:
        raise NotImplementedError("fieldsplit ksp_norm_type must be preconditioned, unpreconditioned or none on both blocks")
    cfg.inner_norm = {"preconditioned": 0, "unpreconditioned": 1, "none": 2}[norms.pop()]
    if cfg.inner_norm == 2:
        # PETSc's KSP_NORM_NONE: no convergence test, exactly ksp_max_it iterations per block solve
        if cfg.inner_ksp_type != _ffi.KSP_CG or not maxits:
            raise NotImplementedError("ksp_norm_type none needs ksp_type cg and a ksp_max_it on both blocks")
    reds = [float(s["pph_reduction"]) for s in subs if "pph_reduction" in s]
    cfg.inner_reduction = max(reds) if reds else 0.0


def translate_options(params: Dict, nonlinear: bool = False) -> Tuple[_ffi.SolverCfg, dict]:
    """PETSc option dict -> (pph_solver_cfg, notes).  Unknown keys that do not change the algebra
    (mat_type, monitors, pc_factor_*) are ignored; unsupported algorithms raise NotImplementedError."""
    params = dict(params or {})
    notes: List[str] = []
    cfg = _ffi.SolverCfg()
    cfg.restart = int(params.get("ksp_gmres_restart", 30))
    cfg.max_it = int(params.get("ksp_max_it", 10000))
    # Firedrake's solver defaults (set_defaults of its variational solvers): ksp_rtol 1e-7 unless the user gives one
    cfg.rtol = float(params.get("ksp_rtol", 1e-7))
    cfg.atol = float(params.get("ksp_atol", 1e-50))
    cfg.inner_ksp_type, cfg.inner_pc_type = _ffi.KSP_CG, _ffi.PC_MG
    cfg.inner_rtol, cfg.inner_atol, cfg.inner_max_it = 1e-10, 1e-50, 50000
    cfg.picard = 0
    cfg.picard_rtol = float(params.get("snes_rtol", 1e-8))
    cfg.picard_atol = float(params.get("snes_atol", 1e-50))
    cfg.picard_max_it = int(params.get("snes_max_it", 50))
    cfg.mg_smooth = int(params.get("pph_mg_smooth", 2))
    info = {"direct_equivalent": False}

    # ... and ksp_type preonly + pc_type lu only when the user sets NEITHER: once pc_type is given, the Krylov
    # method is left to PETSc, whose default is gmres (parity unpinned: the reference's own call sites always merge
    # GMRES_PARAMS or LINEAR_SOLVER_PARAMS, so no golden shows these two defaults)
    ksp = params.get("ksp_type", "gmres" if (nonlinear or "pc_type" in params) else "preonly")
    pc = params.get("pc_type", "lu" if ksp == "preonly" else "ilu")
    if pc == "fieldsplit" and params.get("pc_fieldsplit_type", "multiplicative") != "multiplicative":
        raise NotImplementedError("only pc_fieldsplit_type multiplicative is supported")

    if nonlinear or params.get("pph_picard"):
        snes = params.get("snes_type", "ngs")
        if snes not in ("ngs", "nrichardson", "ksponly", "newtonls"):
            raise NotImplementedError(f"snes_type {snes!r} is not supported")
        cfg.picard = 1
        cfg.ksp_type, cfg.pc_type = _ffi.KSP_GMRES, _ffi.PC_FIELDSPLIT
        subs = [_sub_options(params, 0), _sub_options(params, 1)]
        _inner_cfg(cfg, subs, notes)
        notes.append("block Picard (fixed-stress) sweeps per dpp_delayed_form")
        info["notes"] = notes
        return cfg, info

    if ksp == "preonly" and pc in ("lu", "cholesky"):
        # direct solve of the reference -> iterate to direct-solver accuracy
        cfg.ksp_type, cfg.pc_type = _ffi.KSP_GMRES, _ffi.PC_FIELDSPLIT
        cfg.rtol, cfg.atol, cfg.max_it = _DIRECT_RTOL, 1e-300, 200
        cfg.inner_ksp_type, cfg.inner_pc_type = _ffi.KSP_CG, _ffi.PC_MG
        cfg.inner_rtol, cfg.inner_atol = 1e-12, 1e-300
        cfg.inner_exact = 1
        info["direct_equivalent"] = True
        notes.append("preonly+lu -> field-split GMRES with multigrid-CG block solves to 1e-13")
        info["notes"] = notes
        return cfg, info

    cfg.ksp_type = {"preonly": _ffi.KSP_PREONLY, "cg": _ffi.KSP_CG, "gmres": _ffi.KSP_GMRES,
                    "fgmres": _ffi.KSP_GMRES}.get(ksp, -1)
    if cfg.ksp_type < 0:
        raise NotImplementedError(f"ksp_type {ksp!r} is not supported (preonly, cg, gmres)")
    if pc == "ilu" and int(params.get("pc_factor_levels", 0)) != 0:
        raise NotImplementedError("only pc_factor_levels 0 (ILU(0)) is supported")
    if pc in ("lu", "cholesky"):
        raise NotImplementedError("pc_type lu is only supported with ksp_type preonly (direct-equivalent solve)")
    table = {"none": _ffi.PC_NONE, "jacobi": _ffi.PC_JACOBI, "pph_block2": _ffi.PC_BLOCK2,
             "fieldsplit": _ffi.PC_FIELDSPLIT, "ilu": _ffi.PC_ILU, "pph_cmg": _ffi.PC_CMG}
    if pc not in table:
        raise NotImplementedError(f"pc_type {pc!r} is not supported")
    cfg.pc_type = table[pc]
    if pc == "fieldsplit":
        _inner_cfg(cfg, [_sub_options(params, 0), _sub_options(params, 1)], notes)
    info["notes"] = notes
    return cfg, info


def _apply_bcs(ctx: _ffi.Context, W, bcs: List[fd.DirichletBC]) -> None:
    per_field = {0: (np.zeros(0, np.int64), np.zeros(0)), 1: (np.zeros(0, np.int64), np.zeros(0))}
    for bc in bcs or []:
        V = bc.function_space()
        if getattr(V, "parent", None) is not W:
            raise ValueError("DirichletBC must be built on W.sub(i) of the space being solved")
        per_field[bc.field] = bc.nodes_and_values()
    # a set that is already on the device (same nodes, same values) is not applied again: pph_set_dirichlet drops the
    # assembled system and makes the multigrid hierarchy re-derive its masks
    for f in (0, 1):
        nodes, vals = per_field[f]
        if not ctx.same_dirichlet(f, nodes, vals):
            if isinstance(vals, np.ndarray):
                ctx.set_dirichlet(f, nodes, vals)
            else:
                ctx.set_dirichlet_device(f, nodes, vals)    # (device data: DirichletBC.nodes_and_values)


def degree2_unsupported(cfg: _ffi.SolverCfg, info: dict) -> Optional[str]:
    """Why a translated configuration cannot run on a degree-2 space, or None.  Multigrid there is the block pc_type
    pph_pmg (PC_PMG); mg, and the LU blocks and direct-equivalent solve that stand on it, stay refused."""
    if info.get("direct_equivalent"):
        return "ksp_type preonly + pc_type lu runs as field-split GMRES with multigrid-CG block solves"
    if cfg.pc_type == _ffi.PC_MG:
        return "pc_type mg needs the multigrid hierarchy"
    if cfg.pc_type == _ffi.PC_CMG and not cfg.picard:
        return "pc_type pph_cmg is a cycle on the CG-1 multigrid hierarchy"
    if (cfg.pc_type == _ffi.PC_FIELDSPLIT or cfg.picard) and cfg.inner_pc_type == _ffi.PC_MG:
        what = "Picard" if cfg.picard else "field-split"
        if cfg.inner_exact:
            return f"{what} blocks with pc_type lu run as multigrid-CG block solves"
        return f"{what} blocks with pc_type mg need the multigrid hierarchy"
    return None


_warned_direct = False


def _run(W, model_params: DPPParameters, bcs, solver_parameters: Dict, nonlinear: bool,
         device: Optional[int] = None) -> Solution:
    global _warned_direct
    cfg, info = translate_options(solver_parameters, nonlinear=nonlinear)
    mesh = W.mesh()
    degree = getattr(W.sub(0), "degree", 1)
    if degree != 1:
        # checked before any context exists: a refusal never touches a GPU
        why = degree2_unsupported(cfg, info)
        if why is not None:
            raise NotImplementedError(f"degree-{degree} spaces have no multigrid hierarchy: {why} (use e.g. GMRES + ILU)")
        if mesh.dim == 3 and mesh.distributed:
            raise NotImplementedError("degree-2 spaces are not distributed: build the mesh with comm=fd.COMM_SELF")
        ctx = mesh.context(device, degree=degree)
    else:
        if cfg.pc_type == _ffi.PC_CMG and not cfg.picard and mesh.distributed:
            # (before the context exists, like the degree-2 refusals)
            raise NotImplementedError("pc_type pph_cmg runs on one device: not available on a distributed mesh (build the "
                                      "mesh with comm=fd.COMM_SELF)")
        # this rank's slab + its transport when the mesh is distributed (fd.Mesh); the solver loops are the same
        ctx = mesh.context(device)
    if mesh.distributed:
        if cfg.pc_type == _ffi.PC_ILU or (cfg.inner_pc_type == _ffi.PC_ILU and cfg.pc_type == _ffi.PC_FIELDSPLIT):
            raise NotImplementedError("pc_type ilu is a sequential-elimination preconditioner: not available on a "
                                      "distributed mesh (use fd.UnitCubeMesh(..., comm=fd.COMM_SELF) or another pc_type)")
        tr = mesh.transport
        info["distributed"] = {"rank": mesh.slab.rank, "world": mesh.slab.world, "transport": tr.label,
                               "rccl_error": tr.rccl_error, "owned_planes": [mesh.slab.owned_planes.start,
                                                                             mesh.slab.owned_planes.stop]}
    elif mesh.replicated_because:
        info["replicated"] = mesh.replicated_because
    if info.get("direct_equivalent") and not _warned_direct:
        # an unsupported algorithm never SILENTLY becomes another one - once per process, audibly
        _warned_direct = True
        warnings.warn("ksp_type preonly + pc_type lu (MUMPS) runs as a direct-EQUIVALENT solve on the GPU: field-split GMRES "
                      "with multigrid-CG block solves to 1e-13; iteration_number 1 / residual 0.0 are reported as PETSc's "
                      "preonly does (see Solution.info['notes'])", stacklevel=3)
    _apply_bcs(ctx, W, bcs)
    need_mono = not cfg.picard
    ctx.assemble(float(model_params.k1), float(model_params.k2), float(model_params.beta), float(model_params.mu),
                 monolithic=need_mono)
    try:
        return _solve_and_wrap(ctx, cfg, W, info)
    except _ffi.ConvergenceError:
        # a solve that also failed to converge still says that its block solves stopped short: the cause comes first
        li = getattr(ctx, "last_info", None)
        if li is not None and li.inner_failed:
            warnings.warn(_INNER_FAILED, stacklevel=3)
        raise


_INNER_FAILED = ("a block solve (an on-chip LU-equivalent one included) or the coarsest multigrid solve stopped at its iteration "
                 "limit or broke down: the preconditioner was inexact beyond its tolerance")


def _solve_and_wrap(ctx: _ffi.Context, cfg: _ffi.SolverCfg, W, info: dict) -> Solution:
    if _ffi.shared_runtime():
        # the result stays on the device: copied there into a tensor of torch's allocator (it outlives the next solve and
        # the context); the host sees it on first access (fd.Function)
        _, sinfo, _ = ctx.solve(cfg, fetch=False)
        solution = fd.Function(W, ctx.solution_tensor(), name="dpp_solution")
    else:
        x, sinfo, _ = ctx.solve(cfg, fetch=True)
        solution = fd.Function(W, x, name="dpp_solution")
    info.update(iterations=int(sinfo.iterations), inner_iterations=int(sinfo.inner_iterations),
                residual=float(sinfo.resnorm), rhs_norm=float(sinfo.rhs_norm), timers=ctx.timers(),
                converged=bool(sinfo.converged), inner_failed=bool(sinfo.inner_failed))
    if sinfo.inner_failed:
        # (a direct-equivalent solve reports residual_error 0.0 below: never without this warning when a block solve,
        # on chip or host-driven, ended short of its tolerance)
        warnings.warn(_INNER_FAILED, stacklevel=4)
    if info.get("direct_equivalent"):
        return Solution(solution, 1, 0.0, info)
    return Solution(solution, int(sinfo.iterations), float(sinfo.resnorm), info)


def solve_dpp(W, model_params: DPPParameters, bcs: List[fd.DirichletBC], solver_parameters: Dict = {},
              options_prefix: str = "dpp") -> Solution:
    """Solve the monolithic / preconditioned DPP linear system (reference solver.py:30-76)."""
    if not hasattr(W, "num_sub_spaces") or W.num_sub_spaces() != 2:
        raise ValueError(f"Expected a 2-field MixedFunctionSpace, got {type(W)}")
    dpp_form(W, model_params)  # same guard + form description as the reference
    return _run(W, model_params, bcs, solver_parameters, nonlinear=False)


def solve_dpp_nonlinear(W, model_params: DPPParameters, bcs: List[fd.DirichletBC], solver_parameters: Dict = {},
                        options_prefix: str = "dpp_nonlinear") -> Solution:
    """Fixed-point (Picard) solve of the split system (reference solver.py:79-128): block
    Gauss-Seidel sweeps over the two scales; returns sweeps and the final residual norm."""
    if not hasattr(W, "num_sub_spaces") or W.num_sub_spaces() != 2:
        raise ValueError(f"Expected a 2-field MixedFunctionSpace, got {type(W)}")
    dpp_splitted_form(W, model_params)
    sol = _run(W, model_params, bcs, solver_parameters, nonlinear=True)
    assert isinstance(sol, Solution)
    return sol
