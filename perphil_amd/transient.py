"""
Transient double-porosity/permeability solves: storage terms and theta time stepping on the device.

No reference counterpart: the reference solves the steady state of ``dpp_form`` (``src/perphil/forms/dpp.py:95-132``).  With a
storage coefficient ``S_f > 0`` per network, on the unit box with Dirichlet data constant in time,

    S1 dp1/dt - div(k1/mu grad p1) + beta/mu (p1 - p2) = 0
    S2 dp2/dt - div(k2/mu grad p2) - beta/mu (p1 - p2) = 0

and the theta scheme (``1/2 <= theta <= 1``: backward Euler 1, Crank-Nicolson 1/2) in delta form

    (Sigma M / dt + theta A) d = -F A_unel p^n,      p^{n+1} = p^n + d,      d = 0 on constrained dofs.

``pph_transient_begin`` assembles the step operator once (``pph_assemble_dpp_shifted``), ``pph_transient_steps`` runs the steps
on the device: a matrix-free kernel forms the right-hand side, the solve is the one ``solve_dpp`` would run for the same
``solver_parameters``, one kernel adds the increment.  Single-context meshes, degree 1 and 2.  Every check of the arguments
comes before the first use of a context: a refusal never touches a GPU.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import attr
import numpy as np

from . import _ffi, fd, solver
from .adjoint import _field_values, _mixed_space
from .parameters import DPPParameters


@attr.define(frozen=True)
class TransientSolution:
    """Result of ``solve_dpp_transient``.  ``times``: [steps_done + 1], starting at 0.  ``solution``: the final mixed Function
    (device-resident when asked and possible, like ``Solution.solution``).  ``iterations`` / ``rhs_norms`` /
    ``increment_norms``: per step, the solve's iteration count, ``||b_s||_2`` and ``||d_s||_2``.  ``observations``:
    ``[steps_done + 1, points, 2]`` values of (p1, p2) at ``observe_at`` after every step, step 0 (the initial field with the
    Dirichlet values applied) included, or None.  ``snapshots``: ``{step: Function}`` every ``record_every`` steps (step 0
    and the last step included), empty when ``record_every`` is 0.  ``info``: what ran."""
    times: np.ndarray
    solution: fd.Function = attr.field(eq=False)
    iterations: np.ndarray
    rhs_norms: np.ndarray
    increment_norms: np.ndarray
    observations: Optional[np.ndarray]
    snapshots: Dict[int, fd.Function] = attr.field(factory=dict, eq=False)
    info: dict = attr.field(factory=dict, eq=False)

    @property
    def steps_done(self) -> int:
        return int(self.times.size - 1)


def _pair(v, name: str):
    try:
        a, b = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a pair of numbers, got {v!r}") from None
    return a, b


def _initial_values(W, initial, degree: int):
    """`initial` - a Function on W, a pair (callable or n-array per field), a 2n array or device tensor - as what
    ``adjoint._field_values`` returns.  No context, no device."""
    if isinstance(initial, (tuple, list)):
        if len(initial) != 2:
            raise ValueError("initial must hold one entry per field")
        n = W.sub(0).local_dim()
        X = None
        parts = []
        for f, v in enumerate(initial):
            if callable(v):
                if X is None:
                    X = W.mesh().node_coordinates(degree=degree)
                v = v(X)
            a = np.asarray(v, dtype=np.float64)
            if a.shape != (n,):
                raise ValueError(f"initial[{f}] must give {n} nodal values, got shape {a.shape}")
            parts.append(a)
        return np.concatenate(parts)
    return _field_values(W, initial, "initial")


def solve_dpp_transient(W, model_params: DPPParameters, bcs: List[fd.DirichletBC], initial, dt: float, num_steps: int,
                        storage: Sequence[float] = (1.0, 1.0), theta: float = 1.0, solver_parameters: Dict = {},
                        observe_at=None, record_every: int = 0, steady_tol: float = 0.0,
                        on_device: bool = False) -> TransientSolution:
    """Theta time stepping of the transient DPP model from ``initial`` over ``num_steps`` steps of ``dt`` (see the module
    docstring).  ``solver_parameters`` as for ``solve_dpp`` (a dictionary with ``snes_type`` other than ``ksponly`` as for
    ``solve_dpp_nonlinear``: the Picard presets); ``DPPParameters`` keeps the reference's fields, the storage coefficients
    stand beside it.  ``steady_tol > 0`` stops before the step whose right-hand side has ``||b_s|| <= steady_tol ||b_0||``.
    ``on_device``: the returned Functions stay on the device (needs torch on the library's HIP runtime)."""
    degree = _mixed_space(W)
    mesh = W.mesh()
    if mesh.distributed:
        raise NotImplementedError("transient solves are implemented for single-context meshes: build the mesh with "
                                  "comm=fd.COMM_SELF")
    nonlinear = solver_parameters.get("snes_type", "ksponly") != "ksponly"
    cfg, info = solver.translate_options(solver_parameters, nonlinear=nonlinear)
    if degree != 1:
        why = solver.degree2_unsupported(cfg, info)
        if why is not None:
            raise NotImplementedError(f"degree-{degree} spaces have no multigrid hierarchy: {why} (use e.g. GMRES + ILU)")
    S1, S2 = _pair(storage, "storage")
    if not (S1 > 0 and S2 > 0 and math.isfinite(S1) and math.isfinite(S2)):
        raise ValueError(f"storage coefficients must be finite and > 0, got {(S1, S2)}")
    dt, theta, steady_tol = float(dt), float(theta), float(steady_tol)
    if not (dt > 0 and math.isfinite(dt)):
        raise ValueError(f"dt must be finite and > 0, got {dt}")
    if not 0.5 <= theta <= 1.0:
        raise ValueError(f"theta must lie in [1/2, 1], got {theta}")
    num_steps, record_every = int(num_steps), int(record_every)
    if num_steps < 1:
        raise ValueError(f"num_steps must be >= 1, got {num_steps}")
    if record_every < 0:
        raise ValueError(f"record_every must be >= 0, got {record_every}")
    if math.isnan(steady_tol):
        raise ValueError("steady_tol must be a number")
    p0 = _initial_values(W, initial, degree)
    pts = None
    if observe_at is not None:
        pts = np.ascontiguousarray(observe_at, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != mesh.dim:
            raise ValueError(f"observe_at must have shape [m, {mesh.dim}], got {pts.shape}")
    shared = _ffi.shared_runtime()
    if on_device and not shared:
        _ffi.require_shared_runtime("solve_dpp_transient(on_device=True)")

    # ---- from here on a context is used ------------------------------------------------------------------------------
    ctx = mesh.context(degree=degree) if degree != 1 else mesh.context()
    solver._apply_bcs(ctx, W, bcs)
    ctx.transient_begin(float(model_params.k1), float(model_params.k2), float(model_params.beta), float(model_params.mu),
                        (S1, S2), theta, dt, monolithic=not cfg.picard)
    n = ctx.n
    if shared:
        import torch

        p = p0.clone() if fd._is_tensor(p0) else torch.from_numpy(p0).to(ctx.torch_device())
        p = p.contiguous()
        dpts = None if pts is None else torch.from_numpy(pts).to(ctx.torch_device())
    else:
        p = np.array(p0.cpu().numpy() if fd._is_tensor(p0) else p0, dtype=np.float64)

    def observe():
        if shared:
            ctx.wait_for_torch()
            return np.stack([ctx.eval_points_device(p[f * n:(f + 1) * n], dpts)[0][:, 0].cpu().numpy() for f in (0, 1)], axis=1)
        return np.stack([ctx.eval_points(p[f * n:(f + 1) * n], pts)[0][:, 0] for f in (0, 1)], axis=1)

    def snapshot(step):
        vals = p.clone() if shared else p.copy()
        if shared and not on_device:
            vals = vals.cpu().numpy()
        return fd.Function(W, vals, name=f"dpp_transient_{step}")

    chunk = 1 if pts is not None else (record_every if record_every > 0 else num_steps)
    its: List[int] = []
    bn: List[float] = []
    dn: List[float] = []
    obs = []
    snaps: Dict[int, fd.Function] = {}
    done = 0
    first = True
    converged = True
    while done < num_steps:
        want = min(chunk, num_steps - done)
        if first:
            # step 0 is observed on the field the first step starts from: the constrained entries take the Dirichlet values,
            # as pph_transient_steps sets them first
            first = False
            if pts is not None or record_every > 0:
                _constrain(ctx, W, bcs, p, n, shared)
                if pts is not None:
                    obs.append(observe())
                if record_every > 0:
                    snaps[0] = snapshot(0)
        k, infos, norms = ctx.transient_steps(cfg, p, want, steady_tol=steady_tol, raise_on_diverged=True)
        its += [int(i.iterations) for i in infos]
        converged = converged and all(bool(i.converged) for i in infos)
        bn += [float(v) for v in norms[:, 0]]
        dn += [float(v) for v in norms[:, 1]]
        done += k
        if pts is not None and k > 0:
            obs.append(observe())
        if record_every > 0 and k > 0 and (done % record_every == 0 or done == num_steps or k < want):
            snaps[done] = snapshot(done)
        if k < want:
            break
    final = snapshot(done)
    info.update(steps_done=done, theta=theta, dt=dt, storage=(S1, S2), converged=converged, timers=ctx.timers())
    return TransientSolution(times=dt * np.arange(done + 1), solution=final, iterations=np.array(its, dtype=np.int64),
                             rhs_norms=np.array(bn), increment_norms=np.array(dn),
                             observations=None if pts is None else np.stack(obs), snapshots=snaps, info=info)


def _constrain(ctx, W, bcs, p, n: int, shared: bool) -> None:
    """p = Dirichlet value on the constrained dofs, as pph_transient_steps does first."""
    for bc in bcs or []:
        nodes, vals = bc.nodes_and_values()
        off = bc.field * n
        if shared:
            import torch

            idx = torch.as_tensor(nodes, device=p.device) + off
            p[idx] = vals if fd._is_tensor(vals) else torch.as_tensor(np.asarray(vals, dtype=np.float64), device=p.device)
        else:
            v = vals.cpu().numpy() if fd._is_tensor(vals) else np.asarray(vals, dtype=np.float64)
            p[np.asarray(nodes.cpu().numpy() if fd._is_tensor(nodes) else nodes) + off] = v
