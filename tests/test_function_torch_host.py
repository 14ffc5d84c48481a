"""torch interop of fd.Function / fd.DirichletBC on the host (no GPU needed): tensors in host memory are shared, not
copied, and give the same boundary data as NumPy arrays."""
import gc
import weakref

import numpy as np
import pytest
import torch

import perphil_amd as pa
from perphil_amd import fd


def _mixed_space(nx=3, ny=2):
    mesh = pa.create_mesh(nx, ny, quadrilateral=True)
    _, V = pa.create_function_spaces(mesh)
    return fd.MixedFunctionSpace((V, V))


def test_function_from_cpu_tensor_shares_memory():
    W = _mixed_space()
    t = torch.arange(W.dim(), dtype=torch.float64)
    w = fd.Function(W, t)
    assert not w.on_device
    assert w.vector().ctypes.data == t.data_ptr()
    t[3] = -7.0
    assert w.vector()[3] == -7.0
    w.sub(1).vector()[0] = 42.0                    # views write through to the tensor as well
    assert t[W.sub(0).dim()].item() == 42.0


def test_function_torch_on_host_function_is_zero_copy():
    W = _mixed_space()
    a = np.linspace(0.0, 1.0, W.dim())
    w = fd.Function(W, a)
    t = w.torch()
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device.type == "cpu"
    assert t.data_ptr() == a.ctypes.data and t.shape == (W.dim(),)
    p2 = w.sub(1).torch()
    assert p2.data_ptr() == a[W.sub(0).dim():].ctypes.data
    p2[0] = 5.0
    assert a[W.sub(0).dim()] == 5.0


def test_function_rejects_bad_tensors():
    W = _mixed_space()
    with pytest.raises(ValueError):
        fd.Function(W, torch.zeros(W.dim(), dtype=torch.float32))
    with pytest.raises(ValueError):
        fd.Function(W, torch.zeros(W.dim() + 1, dtype=torch.float64))


def test_dirichlet_bc_with_cpu_tensor_matches_ndarray():
    W = _mixed_space(4, 3)
    mesh = W.mesh()
    X = mesh.node_coordinates()
    vals = 1.0 + X[:, 0] + 2.0 * X[:, 1]
    n_ref, v_ref = fd.DirichletBC(W.sub(1), vals, "on_boundary").nodes_and_values()
    n_t, v_t = fd.DirichletBC(W.sub(1), torch.from_numpy(vals.copy()), "on_boundary").nodes_and_values()
    np.testing.assert_array_equal(np.asarray(n_t), n_ref)
    np.testing.assert_array_equal(np.asarray(v_t), v_ref)
    # a host Function built on a tensor is read like any other Function
    p = fd.Function(W.sub(0), torch.from_numpy(vals.copy()))
    n_f, v_f = fd.DirichletBC(W.sub(0), p, "on_boundary").nodes_and_values()
    np.testing.assert_array_equal(np.asarray(n_f), n_ref)
    np.testing.assert_array_equal(np.asarray(v_f), v_ref)


def test_dropped_function_frees_its_coefficients_at_once():
    # no reference cycle through dat / views: the storage goes with the last reference, without the cyclic collector
    W = _mixed_space()
    w = fd.Function(W, np.arange(W.dim(), dtype=float))
    p1, p2 = w.split()
    d = w.dat.data_ro
    ref = weakref.ref(w.vector())
    del d
    enabled = gc.isenabled()
    gc.disable()
    try:
        del w, p1, p2
        assert ref() is None
    finally:
        if enabled:
            gc.enable()
