"""
Adjoint solves, parameter gradients and a solve that ``loss.backward()`` passes through.

No reference counterpart: the reference's ``solve_dpp`` (``src/perphil/solvers/solver.py:30-76``) solves for given
``k1, k2, beta, mu`` and boundary data; how an output changes with them is left to finite differences.  The operator of
``dpp_form`` (``src/perphil/forms/dpp.py:95-132``) is symmetric, so the adjoint of a functional ``J(p)`` is a solve of the same
assembled system for the right-hand side ``dJ/dp`` (``pph_solve_rhs``: every solver path of ``solve_dpp`` runs it), and three
bilinear forms of (adjoint, solution), computed in one matrix-free pass over the cells (``pph_dpp_bilinear``), are the gradients:

    o0 = lam1^T K p1      o1 = lam2^T K p2      o2 = (lam1 - lam2)^T M (p1 - p2)
    dJ/dk1 = -o0 / mu     dJ/dk2 = -o1 / mu     dJ/dbeta = -o2 / mu     dJ/dmu = (k1 o0 + k2 o1 + beta o2) / mu^2
    dJ/d(boundary value at constrained dof d) = (dJ/dp)_d - (A_unel lam)_d

``dJ/dmu`` is ``lam^T A p``: 0 at a converged solution (without sources the solution does not depend on ``mu``), so its size is
a free check of the whole chain.  Single-context meshes, degree 1 and 2; with torch on the library's HIP runtime everything
stays on the device.  Every check of the arguments comes before the first use of a context: a refusal never touches a GPU.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import attr
import numpy as np

from . import _ffi, fd, solver
from .parameters import DPPParameters
from .solver import Solution


@attr.define(frozen=True)
class Sensitivities:
    """Gradients of a functional J of a DPP solution.  ``k1, k2, beta, mu``: dJ/d(parameter).  ``terms``: ``(o0, o1, o2)``,
    the three bilinear forms they are made of.  ``adjoint``: the Function lambda on W.  ``bcs``: None, or per field a scalar
    Function holding dJ/d(boundary value) on the boundary nodes and 0 elsewhere.  ``info``: the adjoint solve's."""
    k1: float
    k2: float
    beta: float
    mu: float
    terms: Tuple[float, float, float]
    adjoint: fd.Function = attr.field(eq=False)
    bcs: Optional[Tuple[fd.Function, fd.Function]] = attr.field(default=None, eq=False)
    info: dict = attr.field(factory=dict, eq=False)


def _mixed_space(W):
    if not hasattr(W, "num_sub_spaces") or W.num_sub_spaces() != 2:
        raise ValueError(f"Expected a 2-field MixedFunctionSpace, got {type(W)}")
    V1, V2 = W.sub(0), W.sub(1)
    if V1.degree != V2.degree:
        raise ValueError("both pressures must live in spaces of the same degree")
    return V1.degree


def _field_values(W, f, name: str):
    """`f` - a Function on W, a 2n float64 tensor or an array - as a contiguous device tensor or a float64 NumPy array.
    ValueError for a wrong length or dtype; no context and no device is used."""
    n2 = W.local_dim()
    if isinstance(f, fd.Function):
        if f.function_space() is not W:
            raise ValueError(f"{name} must be a Function on the space being solved")
        f = f.torch() if f.on_device else f.vector()
    if fd._is_tensor(f):
        import torch

        if f.dtype != torch.float64 or tuple(f.shape) != (n2,):
            raise ValueError(f"{name} must be float64 with {n2} values, got {f.dtype} of shape {tuple(f.shape)}")
        f = f.detach()
        if f.is_cuda:
            return f.contiguous()
        f = f.numpy()
    a = np.asarray(f)
    if a.dtype != np.float64 or a.shape != (n2,):
        raise ValueError(f"{name} must be float64 with {n2} values, got {a.dtype} of shape {a.shape}")
    return np.ascontiguousarray(a)


def _on_device(ctx, v):
    """Host values uploaded to the context's device when torch shares the library's runtime (results then stay there)."""
    if isinstance(v, np.ndarray) and _ffi.shared_runtime():
        import torch

        return torch.from_numpy(v).to(ctx.torch_device())
    return v


def _prepare(W, solver_parameters: Dict, nonlinear: bool):
    """The checks of solve_dpp that need no context, for a single-context mesh: (cfg, info, degree)."""
    degree = _mixed_space(W)
    mesh = W.mesh()
    if mesh.distributed:
        raise NotImplementedError("adjoint solves are implemented for single-context meshes: build the mesh with "
                                  "comm=fd.COMM_SELF")
    cfg, info = solver.translate_options(solver_parameters, nonlinear=nonlinear)
    if degree != 1:
        why = solver.degree2_unsupported(cfg, info)
        if why is not None:
            raise NotImplementedError(f"degree-{degree} spaces have no multigrid hierarchy: {why} (use e.g. GMRES + ILU)")
    return cfg, info, degree


def _assembled_context(W, model_params: DPPParameters, bcs, cfg, degree: int):
    """The mesh's context with `bcs` applied and the system of `model_params` assembled (a Dirichlet set that is already on
    the device is not applied again; nothing an earlier call left in the context is relied on)."""
    mesh = W.mesh()
    ctx = mesh.context(degree=degree) if degree != 1 else mesh.context()
    solver._apply_bcs(ctx, W, bcs)
    ctx.assemble(float(model_params.k1), float(model_params.k2), float(model_params.beta), float(model_params.mu),
                 monolithic=not cfg.picard)
    return ctx


def _adjoint_solve(W, model_params, bcs, b, cfg, info: dict, degree: int):
    """(ctx, Solution, b where the solve read it) of the solve for the checked right-hand side b."""
    import warnings

    ctx = _assembled_context(W, model_params, bcs, cfg, degree)
    b = _on_device(ctx, b)
    try:
        x, sinfo, _ = ctx.solve_rhs(cfg, b)
    except _ffi.ConvergenceError:
        li = getattr(ctx, "last_info", None)
        if li is not None and li.inner_failed:
            warnings.warn(solver._INNER_FAILED, stacklevel=3)
        raise
    lam = fd.Function(W, x, name="dpp_adjoint")
    info.update(iterations=int(sinfo.iterations), inner_iterations=int(sinfo.inner_iterations),
                residual=float(sinfo.resnorm), rhs_norm=float(sinfo.rhs_norm), timers=ctx.timers(),
                converged=bool(sinfo.converged), inner_failed=bool(sinfo.inner_failed))
    if sinfo.inner_failed:
        warnings.warn(solver._INNER_FAILED, stacklevel=3)
    if info.get("direct_equivalent"):
        return ctx, Solution(lam, 1, 0.0, info), b
    return ctx, Solution(lam, int(sinfo.iterations), float(sinfo.resnorm), info), b


def adjoint_solve(W, model_params: DPPParameters, bcs: List[fd.DirichletBC], rhs, solver_parameters: Dict = {},
                  nonlinear: bool = False) -> Solution:
    """lambda on W with ``F A F lambda = F rhs`` for the system of ``model_params`` and ``bcs`` (F zeroes the constrained dofs;
    lambda is 0 there, and the entries of ``rhs`` there are ignored).  ``rhs``: a Function on W, a 2n float64 tensor or an
    array.  ``solver_parameters`` as for ``solve_dpp`` - with ``nonlinear=True`` as for ``solve_dpp_nonlinear``, so the Picard
    presets run the adjoint too.  The result is device-resident when torch shares the library's HIP runtime;
    ``iteration_number``, ``residual_error`` and ``info`` are what ``solve_dpp`` reports for a solve."""
    cfg, info, degree = _prepare(W, solver_parameters, nonlinear)
    b = _field_values(W, rhs, "rhs")
    return _adjoint_solve(W, model_params, bcs, b, cfg, info, degree)[1]


def sensitivities(W, model_params: DPPParameters, bcs: List[fd.DirichletBC], solution, dJ_dp, solver_parameters: Dict = {},
                  nonlinear: bool = False, wrt_bcs: bool = False) -> Sensitivities:
    """Gradients of a functional J at ``solution`` (the solve of ``model_params`` and ``bcs``), given ``dJ_dp`` = dJ/dp over all
    2n dofs (a Function on W, a tensor or an array, like ``solution``): one adjoint solve with ``solver_parameters``, then the
    bilinear kernel.  ``wrt_bcs``: also dJ/d(boundary values), through the consistent nodal flux of the adjoint
    (``pph_dpp_nodal_flux``).  With device inputs nothing solution-sized goes to the host."""
    cfg, info, degree = _prepare(W, solver_parameters, nonlinear)
    g = _field_values(W, dJ_dp, "dJ_dp")
    p = _field_values(W, solution, "solution")
    ctx, adj, g = _adjoint_solve(W, model_params, bcs, g, cfg, info, degree)
    lam = adj.solution
    k1, k2, beta, mu = (float(getattr(model_params, k)) for k in ("k1", "k2", "beta", "mu"))
    lam_v = lam.torch() if lam.on_device else lam.vector()
    p = _on_device(ctx, p)
    o0, o1, o2 = ctx.dpp_bilinear(lam_v, p)
    out_bcs = None
    if wrt_bcs:
        mesh = W.mesh()
        n = W.sub(0).local_dim()
        r = ctx.dpp_nodal_flux(lam_v, k1, k2, beta, mu)      # A_unel lambda
        # pph_dpp_nodal_flux integrates K and M and keeps them with the mesh; while they are valid pph_assemble_dpp builds the
        # blocks from them instead of by its fused pass (entries differ in the last bit, the on-chip LU-equivalent block
        # solves do not run).  A call that computes gradients must not change what the next solve does: the integrals are
        # marked stale again (their buffers stay), so the next assembly is the one a context without this call would run
        ctx.set_option("invalidate_KM", 1)
        fields = []
        if fd._is_tensor(r):
            import torch

            idx = mesh._boundary_index(r.device, degree)[1]
            for f in (0, 1):
                t = torch.zeros(n, dtype=torch.float64, device=r.device)
                t[idx] = g[f * n + idx] - r[f * n + idx]
                fields.append(fd.Function(W.sub(f), t, name=f"dJ_dbc[{f}]"))
        else:
            idx = mesh.local_boundary_nodes(degree)
            for f in (0, 1):
                t = np.zeros(n, dtype=np.float64)
                t[idx] = g[f * n + idx] - r[f * n + idx]
                fields.append(fd.Function(W.sub(f), t, name=f"dJ_dbc[{f}]"))
        out_bcs = tuple(fields)
    return Sensitivities(k1=-o0 / mu, k2=-o1 / mu, beta=-o2 / mu, mu=(k1 * o0 + k2 * o1 + beta * o2) / (mu * mu),
                         terms=(o0, o1, o2), adjoint=lam, bcs=out_bcs, info=adj.info)


# -- torch autograd ------------------------------------------------------------------------------------------------------
def _scalar(v) -> float:
    return float(v.detach()) if fd._is_tensor(v) else float(v)


def _plain_bcs(W, bcs, values):
    """`bcs` with the data of the fields in `values` ({field: detached tensor}) replaced."""
    out = []
    for bc in bcs or []:
        out.append(fd.DirichletBC(bc.function_space(), values[bc.field]) if bc.field in values else bc)
    return out


def solve_dpp_torch(W, k1, k2, beta, mu, bcs: List[fd.DirichletBC], solver_parameters: Dict = {}, nonlinear: bool = False,
                    adjoint_solver_parameters: Optional[Dict] = None):
    """``solve_dpp`` as a differentiable torch operation: returns the 2n solution tensor (field-major) on the mesh's device.
    ``k1 .. mu``: float64 0-d tensors (any device) or floats; a ``bcs[i].value`` that is a CUDA nodal tensor with
    ``requires_grad`` receives the boundary gradient (zeros at interior nodes).  ``backward`` applies its own boundary sets
    and parameters again, runs ONE adjoint solve - with ``adjoint_solver_parameters``, or the forward options when None - and
    the bilinear kernel: a forward solve with other parameters between forward and backward does not change the gradients."""
    import torch

    _ffi.require_shared_runtime("solve_dpp_torch")
    _prepare(W, solver_parameters, nonlinear)
    adj_params = solver_parameters if adjoint_solver_parameters is None else adjoint_solver_parameters
    _prepare(W, adj_params, nonlinear)
    for v in (k1, k2, beta, mu):
        if fd._is_tensor(v) and (v.dtype != torch.float64 or v.dim() != 0):
            raise ValueError(f"k1, k2, beta, mu must be float64 0-d tensors or floats, got {v.dtype} of shape {tuple(v.shape)}")
    bcs = list(bcs or [])
    tracked = {bc.field: bc.value for bc in bcs
               if fd._is_tensor(bc.value) and bc.value.is_cuda and bc.value.requires_grad}
    fields = sorted(tracked)

    class _Solve(torch.autograd.Function):
        @staticmethod
        def forward(actx, k1_, k2_, beta_, mu_, *bvals):
            vals = {f: v.detach() for f, v in zip(fields, bvals)}
            params = DPPParameters(k1=_scalar(k1_), k2=_scalar(k2_), beta=_scalar(beta_), mu=_scalar(mu_))
            plain = _plain_bcs(W, bcs, vals)
            run = solver.solve_dpp_nonlinear if nonlinear else solver.solve_dpp
            sol = run(W, params, plain, solver_parameters).solution
            p = sol.torch() if sol.on_device else torch.from_numpy(sol.vector()).to(torch.device("cuda", W.mesh().device_index()))
            actx.pph = (params, plain, [(v.device if fd._is_tensor(v) else None) for v in (k1_, k2_, beta_, mu_)])
            actx.save_for_backward(p)
            return p.clone()

        @staticmethod
        def backward(actx, grad):
            params, plain, devs = actx.pph
            (p,) = actx.saved_tensors
            need_bc = any(actx.needs_input_grad[4:])
            s = sensitivities(W, params, plain, p, grad.contiguous(), adj_params, nonlinear, wrt_bcs=need_bc)
            out = [torch.tensor(v, dtype=torch.float64, device=d) if (d is not None and need) else None
                   for v, d, need in zip((s.k1, s.k2, s.beta, s.mu), devs, actx.needs_input_grad[:4])]
            for i, f in enumerate(fields):
                out.append(s.bcs[f].torch() if actx.needs_input_grad[4 + i] else None)
            return tuple(out)

    return _Solve.apply(k1, k2, beta, mu, *[tracked[f] for f in fields])
