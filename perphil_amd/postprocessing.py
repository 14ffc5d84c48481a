"""
Post-processing — mirror of reference ``src/perphil/utils/postprocessing.py``:
``split_dpp_solution`` (:6-31), ``calculate_darcy_velocity_from_pressure`` (:34-63), ``slice_along_x`` (:66-86), ``l2_error`` (:89-105), ``h1_seminorm_error``
(:108-124).  The two error norms run on the device: a Gauss rule per cell on the isoparametric map, with the
manufactured pressure evaluated in closed form at every quadrature point (``pph_error_norms_mms``) or, for any other
exact field, with samples the caller's callable provides at those points (``pph_quadrature_points`` /
``pph_error_norms_sampled``).
"""
from __future__ import annotations

from typing import Optional, Tuple

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
