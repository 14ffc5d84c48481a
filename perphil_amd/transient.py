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

Wells and distributed sources (``Well``, ``DistributedSource``; ``perphil_amd/csrc/pph_sources.hip``) put ``q_f(x, t)`` on the
right of the two equations: with load vectors ``L_k`` constant in time and rates ``r_k(t)`` (``q > 0`` injects) a step solves

    (Sigma M / dt + theta A) d = F (-A_unel p^n + sum_k c[n][k] L_k),    c[n][k] = theta r_k(t_{n+1}) + (1 - theta) r_k(t_n).

``F`` zeroes the constrained dofs: a well on a Dirichlet node pumps into the boundary condition.  Steady-state sources,
time-dependent boundary data and slabs stay out of scope.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

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
    and the last step included), empty when ``record_every`` is 0.  ``info``: what ran.  ``trajectory``: None, or with
    ``record_trajectory`` every state ``[steps_done + 1, 2n]`` (a device tensor when torch shares the library's runtime, else
    an array): what ``transient_sensitivities`` runs backwards over."""
    times: np.ndarray
    solution: fd.Function = attr.field(eq=False)
    iterations: np.ndarray
    rhs_norms: np.ndarray
    increment_norms: np.ndarray
    observations: Optional[np.ndarray]
    snapshots: Dict[int, fd.Function] = attr.field(factory=dict, eq=False)
    info: dict = attr.field(factory=dict, eq=False)
    trajectory: Any = attr.field(default=None, eq=False)
    source_rates: Optional[np.ndarray] = attr.field(default=None, eq=False)   # [num_steps + 1, K] as given, None without sources

    @property
    def steps_done(self) -> int:
        return int(self.times.size - 1)


# -- wells and distributed sources ---------------------------------------------------------------------------------------
@attr.define(frozen=True, eq=False)
class Well:
    """A point source in network ``network`` (0 or 1) at ``point`` ([dim]): the load ``L[node] = phi_node(point)`` on the
    nodes of the cell that holds the point - the transpose of ``Function.at``, with its location rule and tie-breaks.
    ``rate``: a float (constant), ``num_steps + 1`` values at ``t_0 .. t_N`` (array or tensor) or a callable ``t -> float``
    evaluated at those times; ``rate > 0`` injects.  A well on a Dirichlet node pumps into the boundary condition: whatever
    falls on constrained dofs is dropped."""
    point: Any
    rate: Any
    network: int = 0


@attr.define(frozen=True, eq=False)
class DistributedSource:
    """A distributed source ``rate(t) f(x)`` in network ``network``: the consistent load ``M f`` there and 0 in the other
    network.  ``f``: a scalar Function on ``W.sub(network)``'s space, a callable of the node coordinates ``[n, dim]`` or an
    array (or device tensor) of ``n`` nodal values.  ``rate`` as for ``Well``."""
    f: Any
    rate: Any = 1.0
    network: int = 0


@attr.define
class _SourcePlan:
    """What ``sources`` means for a run of N steps, worked out without a context.  The library numbers the dense loads first,
    then the points: ``perm[i]`` is the library's column of the caller's source i."""
    rates: np.ndarray                  # [N + 1, K], the caller's order
    coef: np.ndarray                   # [N, K], the library's order: theta r(t_{s+1}) + (1 - theta) r(t_s)
    perm: np.ndarray
    points: np.ndarray                 # [m, dim]
    fields: np.ndarray                 # [m] int32
    dense: List[Tuple[int, Any]]       # (network, nodal values of f: array or device tensor)


def _rate_values(rate, N: int, dt: float, name: str) -> np.ndarray:
    if callable(rate) and not fd._is_tensor(rate):
        r = np.array([float(rate(dt * j)) for j in range(N + 1)], dtype=np.float64)
    else:
        try:
            r = np.asarray(rate.detach().cpu().numpy() if fd._is_tensor(rate) else rate, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{name}: rate must be a number, {N + 1} values or a callable of t, got {rate!r}") from None
        if r.ndim == 0:
            r = np.full(N + 1, float(r))
    if r.shape != (N + 1,):
        raise ValueError(f"{name}: rate must hold the {N + 1} values at t_0 .. t_N, got shape {r.shape}")
    if not np.all(np.isfinite(r)):
        raise ValueError(f"{name}: rates must be finite")
    return r


def _plan_sources(W, degree: int, sources, N: int, dt: float, theta: float, steady_tol: float = 0.0) -> Optional[_SourcePlan]:
    """Every check of ``sources``; no context, no device."""
    sources = list(sources or [])
    if not sources:
        return None
    mesh = W.mesh()
    n = W.sub(0).local_dim()
    rates, wells, dense, kinds = [], [], [], []
    X = None
    for i, s in enumerate(sources):
        name = f"sources[{i}]"
        if not isinstance(s, (Well, DistributedSource)):
            raise ValueError(f"{name} must be a transient.Well or a transient.DistributedSource, got {type(s)}")
        if s.network not in (0, 1) or isinstance(s.network, bool):
            raise ValueError(f"{name}: network must be 0 or 1, got {s.network!r}")
        r = _rate_values(s.rate, N, dt, name)
        if steady_tol > 0.0 and np.any(r != r[0]):
            raise ValueError(f"{name}: steady_tol > 0 needs rates that are constant over the run - the stop test compares with the "
                             "first right-hand side, which a rate schedule makes meaningless (it may be 0)")
        rates.append(r)
        if isinstance(s, Well):
            pt = np.asarray(s.point.detach().cpu().numpy() if fd._is_tensor(s.point) else s.point, dtype=np.float64).reshape(-1)
            if pt.shape != (mesh.dim,):
                raise ValueError(f"{name}: point must have {mesh.dim} coordinates, got {pt.shape}")
            if fd._outside_unit_box(pt[None], (mesh.nx, mesh.ny, mesh.nz)[:mesh.dim], 1e-12)[0]:
                raise fd.PointNotInDomainError(f"{name}: the point {pt.tolist()} is outside the mesh")
            kinds.append(("w", len(wells)))
            wells.append((pt, int(s.network)))
        else:
            f = s.f
            if isinstance(f, fd.Function):
                V = f.function_space()
                if getattr(V, "num_sub_spaces", lambda: 2)() != 1 or V.mesh() is not mesh or V.degree != degree \
                        or isinstance(V, fd.VectorFunctionSpace):
                    raise ValueError(f"{name}: f must be a scalar Function on the space of W.sub({s.network})")
                f = f.torch() if f.on_device else f.vector()
            elif callable(f) and not fd._is_tensor(f):
                if X is None:
                    X = mesh.node_coordinates(degree=degree)
                f = np.asarray(f(X), dtype=np.float64)
            if fd._is_tensor(f):
                import torch

                if f.dtype != torch.float64 or tuple(f.shape) != (n,):
                    raise ValueError(f"{name}: f must hold {n} float64 nodal values, got {f.dtype} of shape {tuple(f.shape)}")
                f = f.detach().contiguous() if f.is_cuda else f.detach().numpy()
            if not fd._is_tensor(f):
                f = np.ascontiguousarray(f, dtype=np.float64)
                if f.shape != (n,):
                    raise ValueError(f"{name}: f must hold {n} nodal values, got shape {f.shape}")
            kinds.append(("d", len(dense)))
            dense.append((int(s.network), f))
    perm = np.array([j if k == "d" else len(dense) + j for k, j in kinds], dtype=np.int64)
    R = np.stack(rates, axis=1)
    coef = np.empty((N, len(sources)), dtype=np.float64)
    coef[:, perm] = theta * R[1:] + (1.0 - theta) * R[:-1]
    points = np.ascontiguousarray([w[0] for w in wells], dtype=np.float64).reshape(len(wells), mesh.dim)
    return _SourcePlan(rates=R, coef=np.ascontiguousarray(coef), perm=perm, points=points,
                       fields=np.array([w[1] for w in wells], dtype=np.int32), dense=dense)


def _install_sources(ctx, plan: _SourcePlan, shared: bool) -> None:
    """The context's source set from a plan.  M f is formed on the device: the un-eliminated operator with k1 = k2 = 0,
    beta = mu = 1 applied to (f, 0) is (M f, -M f)."""
    n = ctx.n
    loads = []
    if shared:
        import torch

        dev = ctx.torch_device()
        for net, f in plan.dense:
            z = torch.zeros(2 * n, dtype=torch.float64, device=dev)
            z[:n] = f if fd._is_tensor(f) else torch.from_numpy(f).to(dev)
            r = ctx.dpp_nodal_flux(z, 0.0, 0.0, 1.0, 1.0)
            L = torch.zeros(2 * n, dtype=torch.float64, device=dev)
            L[net * n:(net + 1) * n] = r[:n]
            loads.append(L)
        dense = torch.stack(loads).contiguous() if loads else None
        points = torch.from_numpy(plan.points).to(dev) if len(plan.points) else None
    else:
        for net, f in plan.dense:
            z = np.zeros(2 * n, dtype=np.float64)
            z[:n] = f.cpu().numpy() if fd._is_tensor(f) else f
            r = ctx.dpp_nodal_flux(z, 0.0, 0.0, 1.0, 1.0)
            L = np.zeros(2 * n, dtype=np.float64)
            L[net * n:(net + 1) * n] = r[:n]
            loads.append(L)
        dense = np.stack(loads) if loads else None
        points = plan.points if len(plan.points) else None
    if loads:
        ctx.set_option("invalidate_KM", 1)                   # (as transient_sensitivities: the next assembly is unchanged)
    outside = ctx.sources_set(dense, points, plan.fields)
    if outside:
        raise fd.PointNotInDomainError(f"{outside} well(s) lie outside the mesh")


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
                        on_device: bool = False, record_trajectory: bool = False,
                        max_trajectory_bytes: int = 8 << 30, sources=None) -> TransientSolution:
    """Theta time stepping of the transient DPP model from ``initial`` over ``num_steps`` steps of ``dt`` (see the module
    docstring).  ``solver_parameters`` as for ``solve_dpp`` (a dictionary with ``snes_type`` other than ``ksponly`` as for
    ``solve_dpp_nonlinear``: the Picard presets); ``DPPParameters`` keeps the reference's fields, the storage coefficients
    stand beside it.  ``steady_tol > 0`` stops before the step whose right-hand side has ``||b_s|| <= steady_tol ||b_0||``.
    ``on_device``: the returned Functions stay on the device (needs torch on the library's HIP runtime).
    ``record_trajectory``: keep every state in ``TransientSolution.trajectory`` (``(num_steps + 1) 2n`` doubles, refused above
    ``max_trajectory_bytes`` and together with ``steady_tol > 0``; there is no checkpointing).
    ``sources``: None, or a list of ``Well`` and ``DistributedSource``: step s adds ``F sum_k c[s][k] L_k`` to its right-hand
    side, ``c[s][k] = theta r_k(t_{s+1}) + (1 - theta) r_k(t_s)`` (``pph_transient_steps_sources``); ``steady_tol > 0`` then
    needs constant rates.  None or an empty list runs the calls a run without sources runs."""
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
    if record_trajectory:
        if steady_tol > 0.0:
            raise ValueError("record_trajectory records a run of exactly num_steps steps: it cannot be combined with steady_tol > 0")
        nbytes = (num_steps + 1) * W.local_dim() * 8
        if nbytes > int(max_trajectory_bytes):
            raise ValueError(f"the trajectory of {num_steps + 1} states of {W.local_dim()} values takes {nbytes} bytes "
                             f"({nbytes / 2 ** 30:.3g} GiB), more than max_trajectory_bytes = {int(max_trajectory_bytes)}; "
                             "trajectories are not checkpointed")
    p0 = _initial_values(W, initial, degree)
    pts = None
    if observe_at is not None:
        pts = np.ascontiguousarray(observe_at, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != mesh.dim:
            raise ValueError(f"observe_at must have shape [m, {mesh.dim}], got {pts.shape}")
    plan = _plan_sources(W, degree, sources, num_steps, dt, theta, steady_tol)
    shared = _ffi.shared_runtime()
    if on_device and not shared:
        _ffi.require_shared_runtime("solve_dpp_transient(on_device=True)")

    # ---- from here on a context is used ------------------------------------------------------------------------------
    ctx = mesh.context(degree=degree) if degree != 1 else mesh.context()
    solver._apply_bcs(ctx, W, bcs)
    if plan is not None:
        _install_sources(ctx, plan, shared)
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
    traj = None
    try:
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
            # (the coefficient rows of this chunk: every step sees the row it would see in one call over the whole run)
            kw = {} if plan is None else {"coef": plan.coef[done:done + want]}
            if record_trajectory:
                k, infos, norms, rows = ctx.transient_steps(cfg, p, want, steady_tol=steady_tol, raise_on_diverged=True, record=True, **kw)
                if want == num_steps:
                    traj = rows
                else:   # (row `done` is written again with the bits it holds)
                    if traj is None:
                        traj = torch.empty((num_steps + 1, 2 * n), dtype=torch.float64, device=p.device) if shared \
                            else np.empty((num_steps + 1, 2 * n), dtype=np.float64)
                    traj[done:done + k + 1] = rows
            else:
                k, infos, norms = ctx.transient_steps(cfg, p, want, steady_tol=steady_tol, raise_on_diverged=True, **kw)
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
    finally:
        if plan is not None:
            ctx.sources_clear()                              # (the loads are this run's: the context keeps none of them, however it ends)
    final = snapshot(done)
    info.update(steps_done=done, theta=theta, dt=dt, storage=(S1, S2), converged=converged, timers=ctx.timers())
    return TransientSolution(times=dt * np.arange(done + 1), solution=final, iterations=np.array(its, dtype=np.int64),
                             rhs_norms=np.array(bn), increment_norms=np.array(dn),
                             observations=None if pts is None else np.stack(obs), snapshots=snaps, info=info,
                             trajectory=None if traj is None else traj[:done + 1],
                             source_rates=None if plan is None else plan.rates)


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


# -- transient adjoint ---------------------------------------------------------------------------------------------------
@attr.define(frozen=True)
class TransientSensitivities:
    """Gradients of a functional ``J = sum_s j_s(p_s)`` of a transient solve.  ``k1, k2, beta, mu``: dJ/d(parameter) (``mu``
    sets the time scale: not 0 here).  ``storage``: (dJ/dS1, dJ/dS2).  ``initial``: dJ/d(initial field), a Function on W, 0 on
    constrained dofs (their initial values are overwritten by the Dirichlet data).  ``bcs``: None, or per field a scalar
    Function holding dJ/d(boundary value) on the boundary nodes and 0 elsewhere.  ``terms``: ``[N, 5]``, the bilinear forms of
    every backward step (``pph_transient_adjoint``); the gradients are made of their sums in the order N-1 down to 0.
    ``info``: the backward solves'."""
    k1: float
    k2: float
    beta: float
    mu: float
    storage: Tuple[float, float]
    initial: fd.Function = attr.field(eq=False)
    bcs: Optional[Tuple[fd.Function, fd.Function]] = attr.field(default=None, eq=False)
    terms: np.ndarray = attr.field(default=None, eq=False)
    info: dict = attr.field(factory=dict, eq=False)
    source_rates: Optional[np.ndarray] = attr.field(default=None, eq=False)   # [N + 1, K] dJ/dr_k(t_j) with wrt_sources


def _as_kind(v, device):
    """`v` (array or tensor) as a contiguous float64 device tensor on `device`, or as a float64 array when `device` is None."""
    if device is None:
        return np.ascontiguousarray(v.detach().cpu().numpy() if fd._is_tensor(v) else v, dtype=np.float64)
    import torch

    t = v.detach() if fd._is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
    return t.to(device=device, dtype=torch.float64).contiguous()


def transient_sensitivities(W, model_params: DPPParameters, bcs: List[fd.DirichletBC], solution: TransientSolution, dJ_dp=None,
                            dJ_dobs=None, observe_at=None, storage: Sequence[float] = (1.0, 1.0), theta: float = 1.0,
                            dt: float = 1.0, solver_parameters: Dict = {}, adjoint_solver_parameters: Optional[Dict] = None,
                            wrt_bcs: bool = False, sources=None, wrt_sources: bool = False) -> TransientSensitivities:
    """Gradients of ``J = sum_{s=0..N} j_s(p_s)`` over the recorded run ``solution`` (``solve_dpp_transient(...,
    record_trajectory=True)`` with the same ``model_params, bcs, storage, theta, dt``).  ``dJ_dp``: ``[N + 1, 2n]``, the
    derivatives dj_s/dp_s; ``dJ_dobs``: ``[N + 1, m, 2]``, the derivatives with respect to the observations (p1, p2) at
    ``observe_at`` ``[m, dim]`` (turned into nodal loads by the transpose of the point evaluation); at least one of them.
    One backward sweep with one solve per step on the forward operator (``pph_transient_adjoint``), with
    ``adjoint_solver_parameters`` or, when None, ``solver_parameters``.  ``wrt_bcs``: also dJ/d(boundary values).  The call
    assembles the step operator itself: nothing an earlier call left in the context is relied on.
    ``sources``: the sources of the recorded run.  They depend neither on the state nor on the parameters, so the recursion and
    every other gradient are what they are without them (the trajectory carries their effect); ``wrt_sources`` adds
    ``source_rates`` ``[N + 1, K]``, ``dJ/dr_k(t_j) = theta G[j-1][k] + (1 - theta) G[j][k]`` with ``G[s][k] = w_s^T F L_k``
    (``pph_transient_adjoint_sources``; rows of G outside 0 .. N-1 are 0)."""
    degree = _mixed_space(W)
    mesh = W.mesh()
    if mesh.distributed:
        raise NotImplementedError("transient sensitivities are implemented for single-context meshes: build the mesh with "
                                  "comm=fd.COMM_SELF")
    params = solver_parameters if adjoint_solver_parameters is None else adjoint_solver_parameters
    nonlinear = params.get("snes_type", "ksponly") != "ksponly"
    cfg, info = solver.translate_options(params, nonlinear=nonlinear)
    if degree != 1:
        why = solver.degree2_unsupported(cfg, info)
        if why is not None:
            raise NotImplementedError(f"degree-{degree} spaces have no multigrid hierarchy: {why} (use e.g. GMRES + ILU)")
    S1, S2 = _pair(storage, "storage")
    if not (S1 > 0 and S2 > 0 and math.isfinite(S1) and math.isfinite(S2)):
        raise ValueError(f"storage coefficients must be finite and > 0, got {(S1, S2)}")
    dt, theta = float(dt), float(theta)
    if not (dt > 0 and math.isfinite(dt)):
        raise ValueError(f"dt must be finite and > 0, got {dt}")
    if not 0.5 <= theta <= 1.0:
        raise ValueError(f"theta must lie in [1/2, 1], got {theta}")
    traj = getattr(solution, "trajectory", None)
    n2 = W.local_dim()
    if traj is None:
        raise ValueError("solution holds no trajectory: run solve_dpp_transient(..., record_trajectory=True)")
    if len(traj.shape) != 2 or traj.shape[1] != n2 or traj.shape[0] < 2:
        raise ValueError(f"solution.trajectory must have shape [N + 1, {n2}] with N >= 1, got {tuple(traj.shape)}")
    N = int(traj.shape[0]) - 1
    if dJ_dp is None and dJ_dobs is None:
        raise ValueError("give dJ_dp, dJ_dobs or both: without either there is no functional to differentiate")
    if dJ_dp is not None and tuple(dJ_dp.shape) != (N + 1, n2):
        raise ValueError(f"dJ_dp must have shape [{N + 1}, {n2}], got {tuple(dJ_dp.shape)}")
    pts = None
    if dJ_dobs is not None:
        if observe_at is None:
            raise ValueError("dJ_dobs needs observe_at, the points the observations were taken at")
        pts = np.ascontiguousarray(observe_at.detach().cpu().numpy() if fd._is_tensor(observe_at) else observe_at, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != mesh.dim:
            raise ValueError(f"observe_at must have shape [m, {mesh.dim}], got {pts.shape}")
        if tuple(dJ_dobs.shape) != (N + 1, pts.shape[0], 2):
            raise ValueError(f"dJ_dobs must have shape [{N + 1}, {pts.shape[0]}, 2], got {tuple(dJ_dobs.shape)}")
        outside = fd._outside_unit_box(pts, (mesh.nx, mesh.ny, mesh.nz)[:mesh.dim], 1e-12)
        if outside.any():
            raise fd.PointNotInDomainError(f"observe_at[{int(np.argmax(outside))}] is outside the mesh")
    k1, k2, beta, mu = (float(getattr(model_params, k)) for k in ("k1", "k2", "beta", "mu"))
    plan = _plan_sources(W, degree, sources, N, dt, theta)
    if wrt_sources and plan is None:
        raise ValueError("wrt_sources needs sources, the sources of the recorded run")
    shared = _ffi.shared_runtime()

    # ---- from here on a context is used ------------------------------------------------------------------------------
    ctx = mesh.context(degree=degree) if degree != 1 else mesh.context()
    solver._apply_bcs(ctx, W, bcs)
    if wrt_sources:
        _install_sources(ctx, plan, shared)
    ctx.transient_begin(k1, k2, beta, mu, (S1, S2), theta, dt, monolithic=not cfg.picard)
    device = ctx.torch_device() if shared else None
    traj = _as_kind(traj, device)
    g = None if dJ_dp is None else _as_kind(dJ_dp, device)
    ox = None if pts is None else _as_kind(pts, device)
    oc = None if dJ_dobs is None else _as_kind(dJ_dobs, device)
    dJ_drates = None
    if wrt_sources:
        try:
            terms, q0, wsum, infos, done, sg = ctx.transient_adjoint(cfg, traj, g, ox, oc, want_wsum=wrt_bcs, want_src_grad=True)
        finally:
            ctx.sources_clear()
        G = np.zeros((N + 2, sg.shape[1]), dtype=np.float64)      # rows -1 .. N: G[j + 1] = src_grad[j], the caller's order
        G[1:N + 1] = sg[:, plan.perm]
        dJ_drates = theta * G[:N + 1] + (1.0 - theta) * G[1:]
    else:
        terms, q0, wsum, infos, done = ctx.transient_adjoint(cfg, traj, g, ox, oc, want_wsum=wrt_bcs)
    tot = np.zeros(5)
    for s in range(N - 1, -1, -1):
        tot += terms[s]
    O0, O1, O2, O3, O4 = (float(v) for v in tot)
    out_bcs = None
    if wrt_bcs:
        n = n2 // 2
        r = ctx.dpp_nodal_flux(wsum, k1, k2, beta, mu)      # A_unel Wsum
        ctx.set_option("invalidate_KM", 1)                   # (as adjoint.sensitivities: the next assembly is unchanged)
        gsum = g.sum(0) if g is not None else (r * 0.0)
        if oc is not None:
            csum = oc.sum(0)
            parts = [ctx.eval_points_adjoint(ox, csum[:, f].contiguous() if shared else np.ascontiguousarray(csum[:, f]))[0]
                     for f in (0, 1)]
            if shared:
                import torch

                gsum = gsum + torch.cat(parts)
            else:
                gsum = gsum + np.concatenate(parts)
        fields = []
        if shared:
            import torch

            idx = mesh._boundary_index(r.device, degree)[1]
            for f in (0, 1):
                t = torch.zeros(n, dtype=torch.float64, device=r.device)
                t[idx] = gsum[f * n + idx] - r[f * n + idx]
                fields.append(fd.Function(W.sub(f), t, name=f"dJ_dbc[{f}]"))
        else:
            idx = mesh.local_boundary_nodes(degree)
            for f in (0, 1):
                t = np.zeros(n, dtype=np.float64)
                t[idx] = gsum[f * n + idx] - r[f * n + idx]
                fields.append(fd.Function(W.sub(f), t, name=f"dJ_dbc[{f}]"))
        out_bcs = tuple(fields)
    info.update(steps_done=done, iterations=[int(i.iterations) for i in infos], converged=all(bool(i.converged) for i in infos),
                theta=theta, dt=dt, storage=(S1, S2), timers=ctx.timers())
    return TransientSensitivities(k1=-O0 / mu, k2=-O1 / mu, beta=-O2 / mu, mu=(k1 * O0 + k2 * O1 + beta * O2) / (mu * mu),
                                  storage=(-O3 / dt, -O4 / dt), initial=fd.Function(W, q0, name="dJ_dinitial"), bcs=out_bcs,
                                  terms=terms, info=info, source_rates=dJ_drates)


def solve_dpp_transient_torch(W, k1, k2, beta, mu, S1, S2, bcs: List[fd.DirichletBC], initial, dt: float, num_steps: int,
                              theta: float = 1.0, solver_parameters: Dict = {}, observe_at=None,
                              adjoint_solver_parameters: Optional[Dict] = None, sources=None):
    """``solve_dpp_transient`` as a differentiable torch operation.  Returns the observations ``[num_steps + 1, m, 2]`` at
    ``observe_at``, or the final 2n state when ``observe_at`` is None, on the mesh's device.  ``k1 .. S2``: float64 0-d
    tensors (any device) or floats; ``initial``: as for ``solve_dpp_transient`` - when it is a CUDA tensor with
    ``requires_grad`` it receives dJ/d(initial field).  ``backward`` assembles the step operator of its own parameters again
    and runs ONE backward sweep (``transient_sensitivities``) with ``adjoint_solver_parameters``, or the forward options when
    None: a forward solve with other parameters between forward and backward does not change the gradients.
    ``sources``: as for ``solve_dpp_transient``; a ``rate`` that is a float64 tensor with ``requires_grad`` (0-d, or the
    ``num_steps + 1`` values) receives dJ/d(rate) on its own device."""
    import torch

    from .adjoint import _scalar

    _ffi.require_shared_runtime("solve_dpp_transient_torch")
    degree = _mixed_space(W)
    mesh = W.mesh()
    if mesh.distributed:
        raise NotImplementedError("transient solves are implemented for single-context meshes: build the mesh with "
                                  "comm=fd.COMM_SELF")
    for v in (k1, k2, beta, mu, S1, S2):
        if fd._is_tensor(v) and (v.dtype != torch.float64 or v.dim() != 0):
            raise ValueError(f"k1, k2, beta, mu, S1, S2 must be float64 0-d tensors or floats, got {v.dtype} of shape "
                             f"{tuple(v.shape)}")
    pts = None
    if observe_at is not None:
        pts = np.ascontiguousarray(observe_at.detach().cpu().numpy() if fd._is_tensor(observe_at) else observe_at, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != mesh.dim:
            raise ValueError(f"observe_at must have shape [m, {mesh.dim}], got {pts.shape}")
    track_initial = fd._is_tensor(initial) and initial.is_cuda and initial.requires_grad
    n = W.sub(0).local_dim()
    bcs = list(bcs or [])
    sources = list(sources or [])
    tracked_rates = [(i, s.rate) for i, s in enumerate(sources) if fd._is_tensor(getattr(s, "rate", None)) and s.rate.requires_grad]
    for i, r in tracked_rates:
        if r.dtype != torch.float64 or r.dim() > 1:
            raise ValueError(f"sources[{i}]: a rate that takes a gradient must be a float64 tensor, 0-d or [num_steps + 1], got "
                             f"{r.dtype} of shape {tuple(r.shape)}")

    class _Transient(torch.autograd.Function):
        @staticmethod
        def forward(actx, k1_, k2_, beta_, mu_, S1_, S2_, *more):
            params = DPPParameters(k1=_scalar(k1_), k2=_scalar(k2_), beta=_scalar(beta_), mu=_scalar(mu_))
            store = (_scalar(S1_), _scalar(S2_))
            p0 = more[0].detach() if track_initial else initial
            sol = solve_dpp_transient(W, params, bcs, p0, dt, num_steps, storage=store, theta=theta,
                                      solver_parameters=solver_parameters, on_device=True, record_trajectory=True,
                                      sources=sources)
            traj = sol.trajectory
            actx.pph = (params, store, sol, [(v.device if fd._is_tensor(v) else None) for v in (k1_, k2_, beta_, mu_, S1_, S2_)])
            if pts is None:
                return traj[-1].clone()
            ctx = mesh.context(degree=degree) if degree != 1 else mesh.context()
            x = torch.from_numpy(pts).to(traj.device)
            rows = [torch.stack([ctx.eval_points_device(traj[s, f * n:(f + 1) * n].contiguous(), x)[0][:, 0] for f in (0, 1)], dim=1)
                    for s in range(traj.shape[0])]
            return torch.stack(rows)

        @staticmethod
        def backward(actx, grad):
            params, store, sol, devs = actx.pph
            traj = sol.trajectory
            if pts is None:
                g = torch.zeros_like(traj)
                g[-1] = grad
                s = transient_sensitivities(W, params, bcs, sol, dJ_dp=g, storage=store, theta=theta, dt=dt,
                                            solver_parameters=solver_parameters,
                                            adjoint_solver_parameters=adjoint_solver_parameters, sources=sources,
                                            wrt_sources=bool(tracked_rates))
            else:
                s = transient_sensitivities(W, params, bcs, sol, dJ_dobs=grad.contiguous(), observe_at=pts, storage=store,
                                            theta=theta, dt=dt, solver_parameters=solver_parameters,
                                            adjoint_solver_parameters=adjoint_solver_parameters, sources=sources,
                                            wrt_sources=bool(tracked_rates))
            vals = (s.k1, s.k2, s.beta, s.mu, s.storage[0], s.storage[1])
            out = [torch.tensor(v, dtype=torch.float64, device=d) if (d is not None and need) else None
                   for v, d, need in zip(vals, devs, actx.needs_input_grad[:6])]
            at = 6
            if track_initial:
                out.append(s.initial.torch() if actx.needs_input_grad[at] else None)
                at += 1
            for i, r in tracked_rates:      # dJ/dr_i(t_j) on the rate's own device; a 0-d rate stands at every time
                col = s.source_rates[:, i]
                gr = torch.tensor(float(col.sum()), dtype=torch.float64) if r.dim() == 0 else torch.from_numpy(col.copy())
                out.append(gr.to(r.device) if actx.needs_input_grad[at] else None)
                at += 1
            return tuple(out)

    extra = ([initial] if track_initial else []) + [r for _, r in tracked_rates]
    return _Transient.apply(k1, k2, beta, mu, S1, S2, *extra)
