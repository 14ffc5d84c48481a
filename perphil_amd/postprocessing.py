"""
Post-processing — mirror of reference ``src/perphil/utils/postprocessing.py``:
``split_dpp_solution`` (:6-31), ``calculate_darcy_velocity_from_pressure`` (:34-63), ``slice_along_x`` (:66-86), ``l2_error`` (:89-105), ``h1_seminorm_error``
(:108-124); and, without a reference counterpart, the mass balance of a solution: ``integrate``, ``boundary_fluxes``,
``mass_transfer_rate``, ``consistent_fluxes``, ``mass_balance`` (``pph_flux.hip``).  The two error norms run on the device: a Gauss rule per cell on the isoparametric map, with the
manufactured pressure evaluated in closed form at every quadrature point (``pph_error_norms_mms``) or, for any other
exact field, with samples the caller's callable provides at those points (``pph_quadrature_points`` /
``pph_error_norms_sampled``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from . import fd
from .manufactured_solutions import MMSPressure


def split_dpp_solution(dpp_solution: fd.Function) -> Tuple[fd.Function, fd.Function]:
    """(p1_h, p2_h) as independent Functions; ValueError unless the space is a 2-field mixed space."""
    W = dpp_solution.function_space()
    if not hasattr(W, "num_sub_spaces") or W.num_sub_spaces() != 2:
        raise ValueError(f"Expected a 2-field MixedFunctionSpace, got {type(W)}")
    if dpp_solution.on_device:    # (copies on the device: the parts stay where the solution is)
        return (fd.Function(W.sub(0), dpp_solution.sub(0).torch().clone(), name="p1_h"),
                fd.Function(W.sub(1), dpp_solution.sub(1).torch().clone(), name="p2_h"))
    p1 = fd.Function(W.sub(0), dpp_solution.sub(0).vector().copy(), name="p1_h")
    p2 = fd.Function(W.sub(1), dpp_solution.sub(1).vector().copy(), name="p2_h")
    return p1, p2


def calculate_darcy_velocity_from_pressure(pressure_field: fd.Function, conductivity,
                                           velocity_space: Optional[fd.FunctionSpace] = None,
                                           degree: int = 1) -> fd.Function:
    """
    u = -conductivity * grad(p_h), L2-projected onto the CG-1 vector space (``pph_darcy_velocity``:
    node-centred right-hand side kernel + one mass-matrix CG solve per component on the device).
    Coefficients are node-major: ``u.vector().reshape(-1, dim)[node]`` is the velocity at a vertex.
    """
    mesh = pressure_field.function_space().mesh()
    if getattr(pressure_field.function_space(), "degree", 1) != 1:
        raise NotImplementedError("the Darcy velocity of a degree-2 pressure is not implemented")
    if pressure_field.on_device and not mesh.distributed:
        # device in, device out (pph_darcy_velocity_device)
        if velocity_space is None:
            velocity_space = fd.VectorFunctionSpace(mesh, "CG", degree)
        if velocity_space.degree != 1 or velocity_space.mesh() is not mesh:
            raise NotImplementedError("the velocity space must be the CG-1 vector space of the pressure's mesh")
        if not isinstance(conductivity, (int, float, fd.Constant)):
            raise NotImplementedError("conductivity must be a constant")
        u = mesh.context().darcy_velocity_device(pressure_field.torch(), float(conductivity))
        return fd.Function(velocity_space, u, name="velocity")
    if mesh.distributed:
        pressure_field = pressure_field.gather()      # (collective) the projection runs on the serial twin of the mesh
        mesh, velocity_space = pressure_field.function_space().mesh(), None
    if velocity_space is None:
        velocity_space = fd.VectorFunctionSpace(mesh, "CG", degree)
    if velocity_space.degree != 1 or velocity_space.mesh() is not mesh:
        raise NotImplementedError("the velocity space must be the CG-1 vector space of the pressure's mesh")
    if not isinstance(conductivity, (int, float, fd.Constant)):
        raise NotImplementedError("conductivity must be a constant")
    u = mesh.context().darcy_velocity(pressure_field.vector(), float(conductivity))
    return fd.Function(velocity_space, u.reshape(-1), name="velocity")


def slice_along_x(scalar_field: fd.Function, x_value: float) -> Tuple[np.ndarray, np.ndarray]:
    """(y_points, values) of a scalar field along the vertical line x = x_value, any x_value in [0, 1], at the ny + 1 grid
    heights.  On a grid line (every sample a node of the space) the values are the coefficients themselves; otherwise one
    batched point evaluation on the device (``Function.at``)."""
    mesh = scalar_field.function_space().mesh()
    if mesh.dim != 2:
        raise NotImplementedError("slice_along_x is a 2D utility (as in the reference)")
    y_points = np.arange(mesh.ny + 1) / mesh.ny
    if scalar_field._vertex((x_value, 0.0)) is None:
        # between grid lines: one batch (a device-resident field is read where it is)
        X = np.stack([np.full(mesh.ny + 1, float(x_value)), y_points], axis=1)
        return y_points, np.asarray(scalar_field.at(X))
    if scalar_field.on_device:
        # only the slice's values travel: gathered on the device, then copied
        import torch

        idx = [scalar_field._vertex((x_value, y)) for y in y_points]
        t = scalar_field.torch()
        values = t[torch.as_tensor(idx, device=t.device)].cpu().numpy()
        return y_points, values
    values = np.array([scalar_field.at((x_value, y)) for y in y_points])
    return y_points, values


def _norms(numerical: fd.Function, exact_expr, quadrature_points: int):
    """Both norms on the device.  `exact_expr` may be what the reference's UFL argument can be: a manufactured pressure
    (closed form evaluated in the kernel), any callable of point arrays `f(X[m, dim]) -> [m]` (optionally with a
    `.grad(X) -> [m, dim]` attribute; central differences otherwise), a CG-1 `Function` on the same mesh, or a
    `Constant` / number.  A device-resident field is read where it is (no host round trip); on a distributed mesh every
    rank integrates over the cells it owns and the squared norms are summed over the ranks (no gather) whenever torch
    shares the library's runtime."""
    from . import _ffi

    mesh = numerical.function_space().mesh()
    if numerical.on_device or (mesh.distributed and _ffi.shared_runtime()):
        return _norms_device(numerical, exact_expr, quadrature_points)
    if mesh.distributed:
        # post-processing is not on the sharded path: the whole function on the serial twin of the mesh (collective)
        numerical = numerical.gather()
        if isinstance(exact_expr, fd.Function):
            exact_expr = exact_expr.gather()
        mesh = numerical.function_space().mesh()
    ctx = _context(numerical)
    if isinstance(exact_expr, MMSPressure):
        if exact_expr.dim != mesh.dim:
            raise ValueError("exact expression and mesh have different dimensions")
        e = exact_expr
        return ctx.error_norms_mms(e.field, numerical.vector(), e.k1, e.k2, e.beta, e.mu, quadrature_points)
    if isinstance(exact_expr, fd.Function):
        if exact_expr.function_space().mesh() is not mesh:
            raise ValueError("both functions must live on the same mesh")
        diff = np.asarray(numerical.vector(), dtype=np.float64) - np.asarray(exact_expr.vector(), dtype=np.float64)
        return ctx.error_norms_sampled(diff, None, None, min(quadrature_points, _exact_points(numerical)))
    if isinstance(exact_expr, (int, float, fd.Constant)):
        c = float(exact_expr)
        return ctx.error_norms_sampled(numerical.vector(), lambda X: np.full(X.shape[0], c), lambda X: np.zeros_like(X),
                                       quadrature_points)
    if callable(exact_expr):
        return ctx.error_norms_sampled(numerical.vector(), exact_expr, getattr(exact_expr, "grad", None), quadrature_points)
    raise TypeError(f"cannot evaluate an exact expression of type {type(exact_expr).__name__}")


def _context(f: fd.Function):
    """The context of the space `f` lives on (the mesh's CG-1 one, or its degree-2 one)."""
    V = f.function_space()
    deg = getattr(V, "degree", 1)
    return V.mesh().context() if deg == 1 else V.mesh().context(degree=deg)


def _exact_points(f: fd.Function) -> int:
    """Points per direction that integrate the norms of a difference of two functions of f's space exactly: 2-3 for
    CG-1; 3 (Q2) / 4 (P2 on the collapsed rule) for degree 2."""
    return 3 if getattr(f.function_space(), "degree", 1) == 1 else 4


def _device_field(f: fd.Function, ctx):
    """The coefficients of `f` as a device tensor (uploaded when the function lives on the host)."""
    t = f.torch()
    return t if t.is_cuda else t.to(ctx.torch_device())


def _norms_device(numerical: fd.Function, exact_expr, quadrature_points: int, chunk_cells: int = 1 << 16):
    mesh = numerical.function_space().mesh()
    ctx = _context(numerical)
    u = _device_field(numerical, ctx)
    if isinstance(exact_expr, MMSPressure):
        if exact_expr.dim != mesh.dim:
            raise ValueError("exact expression and mesh have different dimensions")
        e = exact_expr
        return ctx.error_norms_mms_device(e.field, u, e.k1, e.k2, e.beta, e.mu, quadrature_points)
    if isinstance(exact_expr, fd.Function):
        if exact_expr.function_space().mesh() is not mesh:
            raise ValueError("both functions must live on the same mesh")
        diff = u - _device_field(exact_expr, ctx)     # (the same IEEE subtraction as the host path's)
        return ctx.error_norms_sampled_device(diff, None, None, min(quadrature_points, _exact_points(numerical)))
    if isinstance(exact_expr, (int, float, fd.Constant)):
        c = float(exact_expr)
        exact, grad = (lambda X: np.full(X.shape[0], c)), (lambda X: np.zeros_like(X))
    elif callable(exact_expr):
        exact, grad = exact_expr, getattr(exact_expr, "grad", None)
    else:
        raise TypeError(f"cannot evaluate an exact expression of type {type(exact_expr).__name__}")
    return ctx.error_norms_sampled_device(u, exact, grad, quadrature_points, chunk_cells=chunk_cells)


def l2_error(numerical: fd.Function, exact_expr, quadrature_points: int = 6) -> float:
    """||numerical - exact||_{L2} (reference postprocessing.py:89-105)."""
    return float(_norms(numerical, exact_expr, quadrature_points)[0])


def h1_seminorm_error(numerical: fd.Function, exact_expr, quadrature_points: int = 6) -> float:
    """|numerical - exact|_{H1} (reference postprocessing.py:108-124)."""
    return float(_norms(numerical, exact_expr, quadrature_points)[1])


# -- mass balance ------------------------------------------------------------------------------------------------------
# Sign conventions.  Sides are numbered as Firedrake numbers UnitSquareMesh / UnitCubeMesh (1: x = 0, 2: x = 1, 3: y = 0,
# 4: y = 1, 5: z = 0, 6: z = 1); a boundary flux is positive OUT of the domain; the transfer T is positive from network 1
# to network 2; a consistent nodal flux r_f[i] is MINUS the outward flux of network f weighted with phi_i.  Every check of
# the arguments comes before the first use of a context: a refusal never touches a GPU.

def _scalar_space(field: fd.Function, what: str):
    V = field.function_space()
    if isinstance(V, (fd.MixedFunctionSpace, fd.VectorFunctionSpace)):
        raise ValueError(f"{what} needs a Function on a scalar CG space, got one on a {type(V).__name__}")
    return V


def _mixed_pair(solution: fd.Function):
    """The two pressure spaces of a mixed solution: ValueError unless it lives on a 2-field mixed space whose fields share
    one mesh and one degree (the two fields are then vectors over the same nodes of one context)."""
    W = solution.function_space()
    if not isinstance(W, fd.MixedFunctionSpace) or W.num_sub_spaces() != 2:
        raise ValueError(f"Expected a Function on a 2-field MixedFunctionSpace, got one on a {type(W).__name__}")
    V1, V2 = W.sub(0), W.sub(1)
    if V1.mesh() is not V2.mesh() or V1.degree != V2.degree:
        raise ValueError("both pressures must live on the same mesh, in spaces of the same degree")
    return V1, V2


def _serial(f: fd.Function) -> fd.Function:
    """`f` itself, or on a distributed mesh the whole function on the mesh's serial twin (collective), as ``at`` does."""
    return f.gather() if f.function_space().mesh().distributed else f


def _coefficients(f: fd.Function):
    """What the context methods take: the device tensor of a device-resident function (read where it is), else the host
    array (uploaded for the call)."""
    return f.torch() if f.on_device else f.vector()


def integrate(field: fd.Function) -> float:
    """``int field dx`` over the unit square / cube, exact for the finite-element function (``pph_integrate``)."""
    _scalar_space(field, "integrate")
    field = _serial(field)
    return float(_context(field).integrate(_coefficients(field)))


def boundary_fluxes(pressure_field: fd.Function, conductivity) -> Dict[int, float]:
    """``{s: int_{side s} -conductivity grad(p_h) . n ds}`` for the sides ``s = 1 .. 2 dim``, outward normal, gradient of
    the cell that owns the facet (``pph_boundary_flux``; the work grows with the boundary, not with the mesh).  For network
    ``f`` of a DPP solution the conductivity is ``k_f / mu``."""
    _scalar_space(pressure_field, "boundary_fluxes")
    if not isinstance(conductivity, (int, float, fd.Constant)):
        raise NotImplementedError("conductivity must be a constant")
    pressure_field = _serial(pressure_field)
    F = _context(pressure_field).boundary_flux(_coefficients(pressure_field), float(conductivity))
    return {s + 1: float(v) for s, v in enumerate(F)}


def mass_transfer_rate(solution: fd.Function, params) -> float:
    """``T = int beta/mu (p1 - p2) dx``: what network 1 hands to network 2 per unit time (the reference's ``xi``,
    src/perphil/forms/dpp.py:27, integrated)."""
    _mixed_pair(solution)
    solution = _serial(solution)
    p1, p2 = solution.subfunctions
    return float(params.beta) / float(params.mu) * (integrate(p1) - integrate(p2))


def consistent_fluxes(solution: fd.Function, params) -> fd.Function:
    """``(r1, r2)`` on W: the residual of the un-eliminated DPP operator, ``r1 = k1/mu K p1 + beta/mu M (p1 - p2)``,
    ``r2 = k2/mu K p2 - beta/mu M (p1 - p2)`` (``pph_dpp_nodal_flux``).  ``r_f[i]`` is minus the outward flux of network f
    weighted with the basis function of node i; ``sum(r1) = T = -sum(r2)`` for any field.  Device-resident when `solution`
    is (no host round trip)."""
    _mixed_pair(solution)
    solution = _serial(solution)
    ctx = _context(solution.sub(0))
    r = ctx.dpp_nodal_flux(_coefficients(solution), float(params.k1), float(params.k2), float(params.beta), float(params.mu))
    return fd.Function(solution.function_space(), r, name="consistent_fluxes")


@dataclass(frozen=True)
class MassBalance:
    """Mass balance of a DPP solution.  ``transfer``: T, network 1 -> 2.  ``outflow_consistent``: per network, minus the sum
    of the consistent nodal fluxes over the boundary nodes.  ``outflow_direct``: per network, ``boundary_fluxes`` of its
    pressure with ``k_f / mu``.  ``imbalance``: ``(outflow_consistent[0] + transfer, outflow_consistent[1] - transfer)``,
    which is the sum of the interior consistent fluxes: rounding for an exactly solved system, the solver's residual
    otherwise."""
    transfer: float
    outflow_consistent: Tuple[float, float]
    outflow_direct: Tuple[Dict[int, float], Dict[int, float]]
    imbalance: Tuple[float, float]


def mass_balance(solution: fd.Function, params) -> MassBalance:
    """Transfer, outflows (consistent and by direct integration of the normal flux) and their imbalance; the boundary set
    is ``Mesh.boundary_nodes(degree)``."""
    V1, _ = _mixed_pair(solution)
    solution = _serial(solution)
    mesh = solution.function_space().mesh()
    n = solution.function_space().sub(0).local_dim()
    T = mass_transfer_rate(solution, params)
    r = consistent_fluxes(solution, params)
    bnd = mesh.boundary_nodes(V1.degree)
    if r.on_device:
        import torch

        t = r.torch()
        idx = torch.as_tensor(bnd, device=t.device)
        out = (-float(t[idx].sum()), -float(t[n + idx].sum()))
    else:
        v = r.vector()
        out = (-float(v[bnd].sum()), -float(v[n + bnd].sum()))
    p1, p2 = solution.subfunctions
    mu = float(params.mu)
    direct = (boundary_fluxes(p1, float(params.k1) / mu), boundary_fluxes(p2, float(params.k2) / mu))
    return MassBalance(T, out, direct, (out[0] + T, out[1] - T))


# -- pathlines -----------------------------------------------------------------------------------------------------------
# Particles carried by v = scale * u_h, u_h a Function on the CG-1 vector space (``pph_trace.hip``: RK4 with a fixed step,
# one lane per particle, the whole batch kept on the device until every particle has ended).  Sides are numbered as above.
# Every check of the arguments comes before the first use of a context.

@dataclass(frozen=True)
class Pathlines:
    """Where a batch of particles went.  ``end [m, dim]``: last position (on the boundary, coordinate exact, for an exited
    particle).  ``time [m]``, ``length [m]``: travel time and arc length up to there.  ``steps [m]``: steps taken.
    ``status [m]``: ``STEP_LIMIT``, ``EXITED``, ``STAGNANT`` (speed <= ``min_speed``) or ``OUTSIDE`` (the seed was not in the
    unit square / cube: NaN end, time and length).  ``side [m]``: the side an exited particle left through (0 otherwise).
    ``paths``: None, or ``[m, n_rec, dim]`` - the position after ``j * record_every`` steps, NaN once the particle has ended
    (a transposed view of the kernel's ``[n_rec, m, dim]``).  ``counts``: particles per status name.  Arrays are NumPy
    arrays, or torch tensors on the device when the seeds or the velocity were there."""
    end: object
    time: object
    length: object
    steps: object
    status: object
    side: object
    paths: object
    counts: Dict[str, int]

    STEP_LIMIT = 0
    EXITED = 1
    STAGNANT = 2
    OUTSIDE = 3


_STATUS_NAMES = ("step_limit", "exited", "stagnant", "outside")


def _trace_arguments(mesh, seeds, dt, max_steps, porosity, min_speed, record_every, chunk):
    """The checks of trace_pathlines that need no velocity (travel_times makes them before it projects one): the seeds as
    an array / device tensor [m, dim], whether they are on the device, and the numbers in their types."""
    dim = mesh.dim
    if mesh.distributed:
        raise NotImplementedError("pathlines are implemented for single-context meshes: build the mesh with comm=fd.COMM_SELF")
    dt, porosity, min_speed = float(dt), float(porosity), float(min_speed)
    if not (np.isfinite(dt) and dt > 0.0):
        raise ValueError(f"dt must be finite and positive, got {dt}")
    if int(max_steps) != max_steps or not 1 <= int(max_steps) < 2 ** 31:
        raise ValueError(f"max_steps must be an integer in [1, 2^31), got {max_steps}")
    if not (np.isfinite(porosity) and porosity > 0.0):
        raise ValueError(f"porosity must be finite and positive, got {porosity}")
    if not min_speed >= 0.0:
        raise ValueError(f"min_speed must not be negative or NaN, got {min_speed}")
    if int(record_every) != record_every or not 0 <= int(record_every) < 2 ** 31:
        raise ValueError(f"record_every must be a non-negative integer, got {record_every}")
    if int(chunk) != chunk or not 1 <= int(chunk) < 2 ** 31:
        raise ValueError(f"chunk must be an integer of at least 1, got {chunk}")
    max_steps, record_every, chunk = int(max_steps), int(record_every), int(chunk)
    dev_seeds = fd._is_tensor(seeds) and seeds.is_cuda
    if fd._is_tensor(seeds):
        import torch

        if seeds.dtype != torch.float64:
            raise ValueError(f"seeds must be float64, got {seeds.dtype}")
        pts = seeds if dev_seeds else seeds.detach().numpy()
    else:
        pts = np.asarray(seeds)
        if pts.dtype.kind not in "fiu":
            raise ValueError(f"seeds must be real numbers, got dtype {pts.dtype}")
        pts = pts.astype(np.float64, copy=False)
    if pts.ndim == 1 and tuple(pts.shape) == (dim,):
        pts = pts.reshape(1, dim)
    if pts.ndim != 2 or pts.shape[1] != dim:
        raise ValueError(f"seeds must be one point of {dim} coordinates or have shape [m, {dim}], got {tuple(pts.shape)}")
    return pts, dev_seeds, dt, max_steps, porosity, min_speed, record_every, chunk


def trace_pathlines(velocity: fd.Function, seeds, dt: float, max_steps: int, *, porosity: float = 1.0,
                    backward: bool = False, min_speed: float = 0.0, record_every: int = 0, chunk: int = 4096) -> Pathlines:
    """Pathlines of the seepage velocity ``velocity / porosity`` (``backward``: of its negative, towards the inflow) from
    ``seeds`` - ``[m, dim]`` as a NumPy array or torch tensor, or one point - by RK4 with the fixed step ``dt``, at most
    ``max_steps`` steps per particle (``pph_trace_pathlines``; the step rule is documented in include/perphil_hip.h).
    ``velocity``: a Function on the CG-1 ``VectorFunctionSpace`` of a single-context mesh, e.g. what
    ``calculate_darcy_velocity_from_pressure`` returns.  Device seeds or a device-resident velocity keep everything on the
    device (the result fields are then CUDA tensors); host inputs give NumPy arrays.  ``chunk``: steps per launch between two
    compactions of the live particles; no result depends on it.  The default leaves paths of up to 4096 steps to one launch:
    on the measured workloads ("Pathlines") every compaction cost more than the idle lanes it removed."""
    V = velocity.function_space()
    mesh = V.mesh()
    if not isinstance(V, fd.VectorFunctionSpace) or getattr(V, "degree", 1) != 1 or V.value_size != mesh.dim:
        raise ValueError(f"trace_pathlines needs a Function on the CG-1 vector space of its mesh (VectorFunctionSpace(mesh, "
                         f"'CG', 1)), got one on a {type(V).__name__} of degree {getattr(V, 'degree', '?')}")
    pts, dev_seeds, dt, max_steps, porosity, min_speed, record_every, chunk = _trace_arguments(
        mesh, seeds, dt, max_steps, porosity, min_speed, record_every, chunk)
    scale = (-1.0 if backward else 1.0) / porosity
    ctx = mesh.context()
    if dev_seeds or velocity.on_device:
        import torch

        u = _device_field(velocity, ctx)
        x = pts if dev_seeds else torch.from_numpy(np.array(pts, dtype=np.float64)).to(ctx.torch_device())   # (a copy: read-only arrays too)
        end, time, length, steps, packed, path, counts = ctx.trace_pathlines_device(
            u.contiguous().reshape(-1), x.contiguous(), scale, dt, max_steps, min_speed, chunk, record_every)
        status, side = packed & 0xFF, packed >> 8
        if path is not None:
            path = path.permute(1, 0, 2)
        if not dev_seeds:
            end, time, length, steps, status, side = (a.cpu().numpy() for a in (end, time, length, steps, status, side))
            path = None if path is None else path.cpu().numpy()
    else:
        end, time, length, steps, packed, path, counts = ctx.trace_pathlines(
            velocity.vector(), np.ascontiguousarray(pts), scale, dt, max_steps, min_speed, chunk, record_every)
        status, side = packed & 0xFF, packed >> 8
        if path is not None:
            path = path.transpose(1, 0, 2)
    return Pathlines(end, time, length, steps, status, side, path, dict(zip(_STATUS_NAMES, (int(c) for c in counts))))


def travel_times(pressure: fd.Function, conductivity, seeds, dt: float, max_steps: int, **kw) -> Pathlines:
    """``trace_pathlines`` of ``calculate_darcy_velocity_from_pressure(pressure, conductivity)``: with ``porosity`` the times
    are seepage travel times of that network, with ``backward=True`` times since the inflow.  A degree-2 pressure is refused,
    as its velocity is."""
    unknown = set(kw) - {"porosity", "backward", "min_speed", "record_every", "chunk"}
    if unknown:
        raise TypeError(f"travel_times got unexpected keyword arguments {sorted(unknown)}")
    V = pressure.function_space()
    if isinstance(V, (fd.MixedFunctionSpace, fd.VectorFunctionSpace)):
        raise ValueError(f"travel_times needs a pressure on a scalar CG-1 space (its velocity lives on the CG-1 vector space), "
                         f"got a Function on a {type(V).__name__}")
    if getattr(V, "degree", 1) != 1:
        raise NotImplementedError("the Darcy velocity of a degree-2 pressure is not implemented (the traced field lives on the "
                                  "CG-1 vector space)")
    _trace_arguments(V.mesh(), seeds, dt, max_steps, kw.get("porosity", 1.0), kw.get("min_speed", 0.0),
                     kw.get("record_every", 0), kw.get("chunk", 4096))
    return trace_pathlines(calculate_darcy_velocity_from_pressure(pressure, conductivity), seeds, dt, max_steps, **kw)
