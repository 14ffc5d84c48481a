"""
Minimal stand-ins for the Firedrake objects that cross the reference's ``solve_dpp`` boundary
(``import firedrake as fd`` in reference ``src/perphil/solvers/solver.py:3``): ``Constant``,
``UnitSquareMesh`` / ``UnitCubeMesh``, ``FunctionSpace`` / ``VectorFunctionSpace`` /
``MixedFunctionSpace``, ``Function``, ``DirichletBC``.  They hold *descriptions* (sizes, kinds,
boundary data); all arithmetic happens in the HIP library behind ``perphil_amd._ffi``.

Numbering (documented, differs from Firedrake's DMPlex numbering which cannot be reproduced):
node (i,j,k) -> i + (nx+1)*(j + (ny+1)*k); mixed dof = field*n + node (field-major, as pinned by
reference ``src/perphil/experiments/iterative_bench.py:323-324``).  Degree-2 spaces (Q2 / P2) number the points of
the lattice refined once the same way: (I,J,K) -> I + (2nx+1)*(J + (2ny+1)*K) at (I/2nx, J/2ny, K/2nz); they live on
the mesh's degree-2 context (``Mesh.context(degree=2)``) and are never distributed.
"""
from __future__ import annotations

import math
import sys
from typing import Callable, Iterable, Optional, Sequence, Tuple, Union

import numpy as np

pi = math.pi


def _is_tensor(x) -> bool:
    """x is a torch.Tensor (without importing torch: no tensor can exist before torch is imported)."""
    t = sys.modules.get("torch")
    return t is not None and isinstance(x, t.Tensor)


CELL_QUAD, CELL_TRI, CELL_HEX, CELL_TET = 0, 1, 2, 3


class Constant:
    """Scalar constant (stand-in for ``fd.Constant``); ``float(c)`` works, arithmetic yields Constants."""

    ufl_shape = ()

    def __init__(self, value):
        self._v = float(value)

    def __float__(self):
        return self._v

    def values(self):
        return np.array([self._v])

    def assign(self, value):
        self._v = float(value)
        return self

    def _b(self, other, op):
        return Constant(op(self._v, float(other)))

    def __add__(self, o): return self._b(o, lambda a, b: a + b)
    def __radd__(self, o): return self._b(o, lambda a, b: b + a)
    def __sub__(self, o): return self._b(o, lambda a, b: a - b)
    def __rsub__(self, o): return self._b(o, lambda a, b: b - a)
    def __mul__(self, o): return self._b(o, lambda a, b: a * b)
    def __rmul__(self, o): return self._b(o, lambda a, b: b * a)
    def __truediv__(self, o): return self._b(o, lambda a, b: a / b)
    def __rtruediv__(self, o): return self._b(o, lambda a, b: b / a)
    def __neg__(self): return Constant(-self._v)
    def __pow__(self, o): return self._b(o, lambda a, b: a ** b)

    def __repr__(self):
        return f"Constant({self._v!r})"


def sqrt(x):
    return Constant(math.sqrt(float(x))) if isinstance(x, Constant) else math.sqrt(x)


COMM_WORLD, COMM_SELF = "world", "self"


class Mesh:
    """Structured unit square / unit cube; lexicographic vertex numbering.

    Under an initialised ``torch.distributed`` group of G > 1 ranks (one process per GPU) a 3D mesh with
    ``comm=COMM_WORLD`` (the default, like Firedrake's) is DISTRIBUTED: rank r holds the cell slab
    ``partition.make_slab(nx, ny, nz, G, r)`` - its owned node planes plus one ghost plane per neighbour - and
    ``context()`` is that slab's device context with its transport attached (RCCL over xGMI with the nccl backend).
    Local node ids are lexicographic inside the slab's box: global id = local id + z_begin * (nx+1)(ny+1).
    2D meshes, meshes with fewer than two cell layers per rank and ``comm=COMM_SELF`` meshes are REPLICATED: every
    rank holds (and solves on) the whole mesh, nothing is communicated.  The decision is taken at first use and kept."""

    def __init__(self, dim: int, kind: int, nx: int, ny: int, nz: int = 0, comm=COMM_WORLD):
        if dim not in (2, 3):
            raise ValueError("dim must be 2 or 3")
        if min(nx, ny) < 1 or (dim == 3 and nz < 1):
            raise ValueError("need at least one cell per direction")
        self.dim, self.kind, self.nx, self.ny, self.nz = dim, kind, int(nx), int(ny), int(nz)
        self.comm = comm
        self._ctx = None  # device context, created on first solve
        self._slab = None          # partition.Slab of this rank once distributed
        self._decided = False      # distribution decided (first use)
        self._dist_args = {}       # distribute(...) keywords: group, device, transport, strict
        self.transport = None      # distributed.Transport once the slab context exists
        self.replicated_because = None

    # -- distribution ---------------------------------------------------------------------------
    def distribute(self, group=None, device=None, transport: str = "auto", strict=None, inject_rccl_failure: bool = False):
        """Optional, before first use: the process group (default: torch.distributed's default group), the device and
        the transport of the slab context.  Without it the defaults apply when the mesh is first used."""
        if self._decided:
            raise RuntimeError("the mesh is already in use: call distribute() right after creating it")
        self._dist_args = dict(group=group, device=device, transport=transport, strict=strict,
                               inject_rccl_failure=inject_rccl_failure)
        return self

    def _decide(self) -> None:
        if self._decided:
            return
        self._decided = True
        if self.comm == COMM_SELF:
            return
        from .distributed import process_group

        pg = process_group()
        if pg is None:
            return
        group = self._dist_args.get("group")
        if group is not None:
            import torch.distributed as dist

            pg = (dist.get_rank(group), dist.get_world_size(group))
            if pg[1] <= 1:
                return
        rank, world = pg
        if self.dim != 3:
            self.replicated_because = "2D meshes are replicated on every rank"
            return
        if self.nz // world < 2:
            self.replicated_because = f"nz = {self.nz} gives fewer than 2 cell layers per rank on {world} ranks"
            return
        from .partition import make_slab

        self._slab = make_slab(self.nx, self.ny, self.nz, world, rank)

    @property
    def slab(self):
        """This rank's ``partition.Slab`` when the mesh is distributed, else None."""
        self._decide()
        return self._slab

    @property
    def distributed(self) -> bool:
        return self.slab is not None

    # -- sizes ----------------------------------------------------------------------------------
    @property
    def node_dims(self) -> Tuple[int, int, int]:
        return self.nx + 1, self.ny + 1, (self.nz + 1 if self.dim == 3 else 1)

    def lattice_dims(self, degree: int = 1) -> Tuple[int, int, int]:
        """Nodes per direction of the degree-`degree` Lagrange space (degree 2: the lattice refined once)."""
        if degree == 1:
            return self.node_dims
        return 2 * self.nx + 1, 2 * self.ny + 1, (2 * self.nz + 1 if self.dim == 3 else 1)

    def num_nodes(self, degree: int = 1) -> int:
        px, py, pz = self.lattice_dims(degree)
        return px * py * pz

    def num_vertices(self) -> int:
        """Global vertex count (like Firedrake's under MPI)."""
        px, py, pz = self.node_dims
        return px * py * pz

    def num_local_vertices(self) -> int:
        """Vertices of this rank's box (owned + ghost planes); = num_vertices() when not distributed."""
        s = self.slab
        return self.num_vertices() if s is None else s.n_local

    def num_cells(self) -> int:
        boxes = self.nx * self.ny * (self.nz if self.dim == 3 else 1)
        return boxes * {CELL_QUAD: 1, CELL_TRI: 2, CELL_HEX: 1, CELL_TET: 6}[self.kind]

    def geometric_dimension(self) -> int:
        return self.dim

    def local_to_global(self, nodes: np.ndarray) -> np.ndarray:
        s = self.slab
        nodes = np.asarray(nodes, dtype=np.int64)
        return nodes if s is None else nodes + s.z_begin * s.plane

    # -- geometry (host side, closed form; only boundary coordinates are needed by the hot path) --
    def node_coordinates(self, nodes: Optional[np.ndarray] = None, degree: int = 1) -> np.ndarray:
        """Coordinates of GLOBAL vertex ids (all vertices if None); degree 2: of the lattice nodes."""
        px, py, _ = self.lattice_dims(degree)
        ids = np.arange(self.num_nodes(degree), dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64)
        i, j = ids % px, (ids // px) % py
        cols = [i / (degree * self.nx), j / (degree * self.ny)]
        if self.dim == 3:
            cols.append((ids // (px * py)) / (degree * self.nz))
        return np.stack(cols, axis=1).astype(np.float64)

    def local_node_coordinates(self, nodes: Optional[np.ndarray] = None, degree: int = 1) -> np.ndarray:
        """Coordinates of LOCAL vertex ids (all local vertices if None); degree-2 nodes are never distributed."""
        if degree != 1:
            return self.node_coordinates(nodes, degree)
        if nodes is None:
            nodes = np.arange(self.num_local_vertices(), dtype=np.int64)
        return self.node_coordinates(self.local_to_global(nodes))

    def boundary_nodes(self, degree: int = 1) -> np.ndarray:
        """Sorted GLOBAL vertex ids (degree 2: lattice node ids) with the "on_boundary" marker."""
        px, py, pz = self.lattice_dims(degree)
        if self.dim == 2:
            m = np.zeros((py, px), dtype=bool)
            m[0, :] = m[-1, :] = True
            m[:, 0] = m[:, -1] = True
        else:
            m = np.zeros((pz, py, px), dtype=bool)
            m[0] = m[-1] = True
            m[:, 0, :] = m[:, -1, :] = True
            m[:, :, 0] = m[:, :, -1] = True
        return np.nonzero(m.ravel())[0].astype(np.int64)

    def local_boundary_nodes(self, degree: int = 1) -> np.ndarray:
        """Sorted LOCAL vertex ids on the boundary of the unit square / cube (ghost planes included: their Dirichlet
        values enter the lifting of the owned rows next to them)."""
        if degree != 1:
            return self.boundary_nodes(degree)
        s = self.slab
        return self.boundary_nodes() if s is None else s.boundary_local()[0]

    def context(self, device: Optional[int] = None, degree: int = 1):
        """Device context holding this mesh - this rank's slab with its transport when the mesh is distributed
        (cell->dof map, operators and the multigrid hierarchy are cached there).  ``degree=2``: the context of the
        degree-2 nodes (whole mesh, CSR operators), cached per device next to the CG-1 one and independent of it."""
        from . import _ffi

        if degree != 1:
            return self._lagrange_context(device, degree)
        s = self.slab
        if device is None:
            device = self._dist_args.get("device")
        if device is None:
            if self._ctx is not None:
                return self._ctx
            if s is not None:
                from .distributed import default_device

                device = default_device()
            else:
                device = 0
        if self._ctx is None or self._ctx.device != device:
            ctx = _ffi.Context(device)
            if s is None:
                ctx.mesh_build(self.dim, self.kind, self.nx, self.ny, self.nz)
            else:
                from .distributed import attach_transport

                ctx.mesh_build(3, self.kind, s.nx, s.ny, s.nz, s.z_begin, s.z_count, s.ghost_lo, s.ghost_hi)
                a = self._dist_args
                self.transport = attach_transport(ctx, a.get("group"), a.get("transport", "auto"), a.get("strict"),
                                                  a.get("inject_rccl_failure", False))
            self._ctx = ctx
        return self._ctx

    def _lagrange_context(self, device: Optional[int], degree: int):
        from . import _ffi

        if degree != 2:
            raise NotImplementedError(f"Lagrange degree {degree}: degrees 1 and 2 are implemented")
        if self.distributed:
            raise NotImplementedError("degree-2 spaces are not distributed: build the mesh with comm=fd.COMM_SELF")
        if device is None:
            device = self.device_index()
        cache = self.__dict__.setdefault("_ctx_deg", {})
        ctx = cache.get((degree, device))
        if ctx is None:
            ctx = _ffi.Context(device)
            ctx.mesh_build_lagrange(self.dim, self.kind, self.nx, self.ny, self.nz, degree)
            cache[(degree, device)] = ctx
        return ctx

    def device_index(self) -> int:
        """The device ``context()`` runs on (or will, when it does not exist yet)."""
        if self._ctx is not None:
            return self._ctx.device
        device = self._dist_args.get("device")
        if device is not None:
            return int(device)
        if self.slab is not None:
            from .distributed import default_device

            return default_device()
        return 0

    def _boundary_index(self, device, degree: int = 1):
        """(local boundary nodes, the same as an int64 tensor on `device`, their global ids as one): kept per device and
        degree."""
        cache = self.__dict__.setdefault("_bnd_index", {})
        key = str(device) if degree == 1 else (str(device), degree)
        if key not in cache:
            import torch

            nodes = self.local_boundary_nodes(degree)
            glob = self.local_to_global(nodes) if degree == 1 else nodes
            cache[key] = (nodes, torch.as_tensor(nodes, device=device), torch.as_tensor(glob, device=device))
        return cache[key]

    def serial_twin(self) -> "Mesh":
        """The same mesh held whole by this process (COMM_SELF): where gathered functions live."""
        if not self.distributed:
            return self
        if getattr(self, "_twin", None) is None:
            self._twin = Mesh(self.dim, self.kind, self.nx, self.ny, self.nz, comm=COMM_SELF)
        return self._twin


def UnitSquareMesh(nx: int, ny: int, quadrilateral: bool = False, comm=COMM_WORLD, **_ignored) -> Mesh:
    """``fd.UnitSquareMesh``: quads, or triangles with the "left" diagonal (Firedrake's default)."""
    return Mesh(2, CELL_QUAD if quadrilateral else CELL_TRI, nx, ny, comm=comm)


def UnitCubeMesh(nx: int, ny: int, nz: int, hexahedral: bool = False, comm=COMM_WORLD, **_ignored) -> Mesh:
    """``fd.UnitCubeMesh``: hexes, or six Kuhn tetrahedra per cube; distributed by cell slabs along z under an
    initialised torch.distributed group (class Mesh)."""
    return Mesh(3, CELL_HEX if hexahedral else CELL_TET, nx, ny, nz, comm=comm)


class FunctionSpace:
    """Continuous Lagrange scalar space: CG-1 (one dof per mesh vertex) or CG-2 (Q2 / P2: one dof per point of the
    lattice refined once, see the module docstring)."""

    def __init__(self, mesh: Mesh, family: str = "CG", degree: int = 1, name: Optional[str] = None):
        if family not in ("CG", "Lagrange", "P", "Q") or degree not in (1, 2):
            raise NotImplementedError("the MI355X path implements the conforming CG-1 and CG-2 pressure spaces only")
        self._mesh, self.family, self.degree, self.name = mesh, "CG", int(degree), name
        self.index: Optional[int] = None
        self.parent: Optional["MixedFunctionSpace"] = None

    def mesh(self) -> Mesh:
        return self._mesh

    def dim(self) -> int:
        """Global dof count (what Firedrake's ``V.dim()`` reports under MPI as well)."""
        return self._mesh.num_vertices() if self.degree == 1 else self._mesh.num_nodes(self.degree)

    def local_dim(self) -> int:
        """Dofs this rank stores (owned + ghost planes of its slab); = dim() when the mesh is not distributed (and for
        degree 2, which is never distributed)."""
        return self._mesh.num_local_vertices() if self.degree == 1 else self._mesh.num_nodes(self.degree)

    def num_sub_spaces(self) -> int:
        return 1

    def __mul__(self, other: "FunctionSpace") -> "MixedFunctionSpace":
        return MixedFunctionSpace((self, other))


class VectorFunctionSpace(FunctionSpace):
    """CG-1 vector space (velocity space U of ``create_function_spaces``; not on the hot path)."""

    def __init__(self, mesh: Mesh, family: str = "CG", degree: int = 1, name: Optional[str] = None):
        if degree != 1:
            raise NotImplementedError("the MI355X path implements the CG-1 vector space only")
        super().__init__(mesh, family, degree, name)
        self.value_size = mesh.dim

    def dim(self) -> int:
        return self._mesh.num_vertices() * self.value_size

    def local_dim(self) -> int:
        return self._mesh.num_local_vertices() * self.value_size


class _IndexedSubSpace(FunctionSpace):
    def __init__(self, parent: "MixedFunctionSpace", index: int, base: FunctionSpace):
        super().__init__(base.mesh(), base.family, base.degree, base.name)
        self.parent, self.index = parent, index


class MixedFunctionSpace:
    """W = V x V; dofs field-major."""

    def __init__(self, spaces: Sequence[FunctionSpace]):
        spaces = tuple(spaces)
        if len(spaces) < 1:
            raise ValueError("need at least one sub space")
        m = spaces[0].mesh()
        if any(s.mesh() is not m for s in spaces):
            raise ValueError("all sub spaces must live on the same mesh")
        self._subs = tuple(_IndexedSubSpace(self, i, s) for i, s in enumerate(spaces))

    def num_sub_spaces(self) -> int:
        return len(self._subs)

    def sub(self, i: int) -> FunctionSpace:
        return self._subs[i]

    def __iter__(self):
        return iter(self._subs)

    def mesh(self) -> Mesh:
        return self._subs[0].mesh()

    def dim(self) -> int:
        return sum(s.dim() for s in self._subs)

    def local_dim(self) -> int:
        return sum(s.local_dim() for s in self._subs)


class _Storage:
    """The coefficients of a Function and of all its views: a host ndarray, or a float64 torch tensor in the memory of the
    mesh's device.  Device data moves to the host once, on the first host access of any view (the context's pinned result
    pool takes it when the mesh has one); from then on the host array is authoritative and the tensor is dropped."""

    __slots__ = ("host", "dev", "mesh")

    def __init__(self, host=None, dev=None, mesh=None):
        self.host, self.dev, self.mesh = host, dev, mesh

    def to_host(self) -> np.ndarray:
        if self.host is None:
            from . import _ffi

            self.host = _ffi.tensor_to_host(self.dev, self.mesh._ctx)
            self.dev = None
        return self.host


class _View:
    """The slice [off, off + n) of a _Storage that a Function and its ``dat`` read (no reference back to the Function: a
    dropped Function, and a device result with it, is freed at once, not by the cyclic garbage collector)."""

    __slots__ = ("st", "off", "n", "hv")

    def __init__(self, st: _Storage, off: int, n: int):
        self.st, self.off, self.n, self.hv = st, off, n, None

    def host(self) -> np.ndarray:
        v = self.hv
        if v is None:
            a = self.st.to_host()
            v = a if (self.off == 0 and self.n == a.shape[0]) else a[self.off:self.off + self.n]
            self.hv = v
        return v

    def owned(self, slab, nfields: int) -> np.ndarray:
        """Owned entries, field-major (a copy when `slab` is set, the host vector itself otherwise)."""
        val = self.host()
        if slab is None:
            return val
        nl = slab.n_local
        return np.concatenate([val[f * nl:(f + 1) * nl][slab.owned_local] for f in range(nfields)])


class _Dat:
    def __init__(self, view: _View, slab, nfields: int):
        self._view, self._slab, self._nf = view, slab, nfields
        self._owned = None

    @property
    def data(self):
        if self._slab is None:
            return self._view.host()
        if self._owned is None:
            self._owned = self._view.owned(self._slab, self._nf)
        return self._owned

    @property
    def data_ro(self):
        return self.data


class Function:
    """Nodal coefficient vector on a (mixed) space; ``sub(i)`` / ``subfunctions`` are views.

    On a distributed mesh the vector is this rank's LOCAL one (field-major over the slab's box, ghost planes
    included, as the device holds it); ``owned()`` drops the ghost planes, ``gather()`` returns the whole function on
    the mesh's serial twin on every rank (``dat.data_ro`` is the owned part, as in Firedrake under MPI).

    ``val`` may be a NumPy array, a 1-D float64 torch tensor in host memory (shared, not copied) or one on the mesh's
    device: the function is then DEVICE-RESIDENT (``on_device``) - as the result of a solve is - and its data stay in GPU
    memory until host code asks for them (``vector()``, ``dat.data``, ``owned()``, ``at()``, ``assign()``,
    ``interpolate()``, ``gather()``), which moves them to the host once for all views.  ``torch()`` hands the storage to
    torch code without a copy."""

    def __init__(self, space, val=None, name: Optional[str] = None, _view=None):
        self._space, self.name = space, name
        mesh = space.mesh()
        if _view is not None:
            self._v = _view
        else:
            n = space.local_dim()
            if val is None:
                val = np.zeros(n, dtype=np.float64)
            st = None
            if _is_tensor(val):
                import torch

                if val.dtype != torch.float64 or val.dim() != 1:
                    raise ValueError(f"a tensor of coefficients must be 1-D float64, got {val.dtype} of shape {tuple(val.shape)}")
                if val.is_cuda:
                    from . import _ffi

                    _ffi.require_shared_runtime("a Function on device data")
                    if val.device.index != mesh.device_index() or not val.is_contiguous():
                        raise ValueError(f"device coefficients must be contiguous and on cuda:{mesh.device_index()}, the "
                                         f"mesh's device (got {val.device})")
                    if tuple(val.shape) != (n,):
                        raise ValueError(f"expected {n} coefficients, got {tuple(val.shape)}")
                    st = _Storage(dev=val.detach(), mesh=mesh)
                else:
                    val = val.detach().numpy()        # host tensor: its memory is the array's
            if st is None:
                if val.shape != (n,):
                    raise ValueError(f"expected {n} coefficients, got {val.shape}")
                st = _Storage(host=val, mesh=mesh)
            self._v = _View(st, 0, n)
        self.dat = _Dat(self._v, mesh.slab, len(self._fields()))

    def function_space(self):
        return self._space

    @property
    def on_device(self) -> bool:
        """True while the coefficients live in GPU memory only."""
        return self._v.st.dev is not None

    def _host(self) -> np.ndarray:
        return self._v.host()

    def vector(self) -> np.ndarray:
        return self._host()

    def torch(self):
        """The coefficients as a torch tensor, without a copy: a CUDA tensor (a view of the storage) while the function is
        device-resident, ``torch.from_numpy(vector())`` otherwise.  Torch's current stream is already ordered after the
        library's writes into it."""
        v = self._v
        dev = v.st.dev
        if dev is None:
            import torch

            return torch.from_numpy(self.vector())
        return dev if (v.off == 0 and v.n == dev.shape[0]) else dev[v.off:v.off + v.n]

    def _fields(self):
        sp = self._space
        return [sp.sub(i) for i in range(sp.num_sub_spaces())] if isinstance(sp, MixedFunctionSpace) else [sp]

    def owned(self) -> np.ndarray:
        """Owned entries, field-major (a copy when the mesh is distributed, the vector itself otherwise)."""
        return self._v.owned(self._space.mesh().slab, len(self._fields()))

    def gather(self) -> "Function":
        """The whole function on the mesh's serial twin, on every rank (collective; small runs, tests and
        post-processing - error norms, ``at``, slices - not the hot path)."""
        mesh = self._space.mesh()
        if not mesh.distributed:
            return self
        from .distributed import gather_field_major

        full = gather_field_major(mesh.slab, self._host(), mesh._dist_args.get("group"))
        twin = mesh.serial_twin()
        fields = self._fields()
        V = FunctionSpace(twin, "CG", 1)
        space = MixedFunctionSpace([V] * len(fields)) if isinstance(self._space, MixedFunctionSpace) else V
        return Function(space, full, name=self.name)

    def sub(self, i: int) -> "Function":
        if not isinstance(self._space, MixedFunctionSpace):
            raise IndexError("not a mixed function")
        off = sum(self._space.sub(k).local_dim() for k in range(i))
        V = self._space.sub(i)
        return Function(V, name=f"{self.name or 'w'}[{i}]", _view=_View(self._v.st, self._v.off + off, V.local_dim()))

    @property
    def subfunctions(self) -> Tuple["Function", ...]:
        return tuple(self.sub(i) for i in range(self._space.num_sub_spaces()))

    def split(self) -> Tuple["Function", ...]:
        return self.subfunctions

    def assign(self, other) -> "Function":
        self._host()[:] = other.vector() if isinstance(other, Function) else float(other)
        return self

    def interpolate(self, expr) -> "Function":
        self._host()[:] = evaluate(expr, self._space.mesh(), None, getattr(self._space, "degree", 1))
        return self

    def at(self, arg, dont_raise: bool = False, tolerance: Optional[float] = None):
        """Value at any point of the domain, or at a batch of points (``fd.Function.at``).

        ``arg``: one point (a sequence of ``dim`` numbers) or an array / torch tensor of shape ``[m, dim]``.  One point
        gives a ``float``, a batch an array ``[m]``; on a vector space ``[ncomp]`` / ``[m, ncomp]``; a mixed function gives
        a tuple with one such entry per sub-function, as in Firedrake.  A single point that coincides with a node of a
        scalar space (within 1e-9 lattice units) returns that coefficient itself.  Everything else is evaluated on the
        device (``pph_eval_points``): a device tensor of points gives a device tensor, and a device-resident function is
        read where it is - host points then cost a copy of the points and of the results only.

        ``tolerance`` (default 1e-12) is in box-local units: a point further outside the unit square / cube raises
        ``PointNotInDomainError`` naming the first such point - for host points before any GPU work - unless
        ``dont_raise``: its values are then NaN.  On a distributed mesh the function is gathered first (collective)."""
        return self._evaluate(arg, False, dont_raise, tolerance)

    def gradient_at(self, arg, dont_raise: bool = False, tolerance: Optional[float] = None):
        """Gradient of the function at a point or a batch of points, with the rules of ``at``: ``[dim]`` / ``[m, dim]`` on a
        scalar space, ``[ncomp, dim]`` / ``[m, ncomp, dim]`` on a vector space, a tuple on a mixed function.  The gradient is
        that of the cell the point is located in (on a face shared by cells: the upper box, then the lowest sub-cell index).
        Firedrake has no counterpart of this method: there one evaluates ``grad(u)`` through an interpolation or
        projection first; here ``-k * p.gradient_at(X)`` is the Darcy flux of a pressure of any degree at any point."""
        return self._evaluate(arg, True, dont_raise, tolerance)

    def _evaluate(self, arg, gradient: bool, dont_raise: bool, tolerance: Optional[float]):
        mesh = self._space.mesh()
        dim = mesh.dim
        tol = 1e-12 if tolerance is None else float(tolerance)
        if not 0.0 <= tol < 0.5:
            raise ValueError("tolerance must be in [0, 0.5) box-local units")
        mixed = isinstance(self._space, MixedFunctionSpace)
        dev_points = _is_tensor(arg) and arg.is_cuda
        if dev_points:
            pts, single = arg, False
            if pts.dim() != 2 or pts.shape[1] != dim:
                raise ValueError(f"points must have shape [m, {dim}], got {tuple(pts.shape)}")
        else:
            pts = np.asarray(arg.detach().numpy() if _is_tensor(arg) else arg, dtype=np.float64)
            single = pts.ndim == 1
            if (single and pts.shape != (dim,)) or (not single and (pts.ndim != 2 or pts.shape[1] != dim)):
                raise ValueError(f"expected one point of {dim} coordinates or an array [m, {dim}], got shape {pts.shape}")
            if single and not gradient and not mixed and not isinstance(self._space, VectorFunctionSpace):
                v = self._vertex(pts)
                if v is not None:      # a node of the space: the coefficient itself
                    f = self.gather() if mesh.distributed else self
                    return float(f._host()[v])
            pts = np.ascontiguousarray(pts.reshape(-1, dim))
            outside = _outside_unit_box(pts, (mesh.nx, mesh.ny, mesh.nz)[:dim], tol)
            if outside.any() and not dont_raise:
                k = int(np.argmax(outside))
                raise PointNotInDomainError(f"point {tuple(float(c) for c in pts[k])} (index {k}) is outside the unit "
                                            f"{'square' if dim == 2 else 'cube'} by more than the tolerance {tol:g}")
        if mesh.distributed:
            return self.gather()._evaluate(arg, gradient, dont_raise, tolerance)
        parts = self.subfunctions if mixed else (self,)
        if not dev_points and outside.all():      # (nothing to evaluate: no context, no device call)
            res = [np.full(f._result_shape(pts.shape[0], gradient), np.nan) for f in parts]
        else:
            res = [f._evaluate_field(pts, gradient, tol, dont_raise) for f in parts]
        if single:
            res = [float(r[0]) if r.ndim == 1 else r[0] for r in res]
        return tuple(res) if mixed else res[0]

    def _result_shape(self, m: int, gradient: bool):
        dim = self._space.mesh().dim
        nc = (getattr(self._space, "value_size", None),) if isinstance(self._space, VectorFunctionSpace) else ()
        return (m,) + nc + ((dim,) if gradient else ())

    def _evaluate_field(self, pts, gradient: bool, tol: float, dont_raise: bool):
        """One (vector or scalar) field at host points (ndarray, checked) or device points (tensor)."""
        V = self._space
        mesh = V.mesh()
        deg = getattr(V, "degree", 1)
        ctx = mesh.context() if deg == 1 else mesh.context(degree=deg)
        ncomp = V.value_size if isinstance(V, VectorFunctionSpace) else 1
        dev_points = _is_tensor(pts)
        if dev_points or self.on_device:
            import torch

            t = self.torch()
            u = t if t.is_cuda else t.to(ctx.torch_device())
            x = pts if dev_points else torch.from_numpy(pts).to(ctx.torch_device())
            val, grad, nout = ctx.eval_points_device(u.contiguous(), x.contiguous(), ncomp, gradient, tol)
            if nout and not dont_raise:     # (device points: only the kernel knows; the same rule names the first one)
                k = int(torch.nonzero(_outside_unit_box_device(x, (mesh.nx, mesh.ny, mesh.nz)[:mesh.dim], tol))[0])
                raise PointNotInDomainError(f"point {tuple(x[k].tolist())} (index {k}) is outside the unit "
                                            f"{'square' if mesh.dim == 2 else 'cube'} by more than the tolerance {tol:g}")
            out = (grad if gradient else val).reshape(self._result_shape(x.shape[0], gradient))
            return out if dev_points else out.cpu().numpy()
        val, grad, _ = ctx.eval_points(self._host(), pts, ncomp, gradient, tol)
        return (grad if gradient else val).reshape(self._result_shape(pts.shape[0], gradient))

    def _vertex(self, point: Sequence[float]) -> Optional[int]:
        """Index of the node of the space `point` coincides with (within 1e-9 lattice units), or None."""
        mesh = self._space.mesh()
        deg = getattr(self._space, "degree", 1)
        idx = []
        for c, nc in zip(point, (deg * mesh.nx, deg * mesh.ny, deg * mesh.nz)[: mesh.dim]):
            t = c * nc
            if not (abs(t - round(t)) <= 1e-9 and 0 <= round(t) <= nc):
                return None
            idx.append(int(round(t)))
        px, py, _ = mesh.lattice_dims(deg)
        return idx[0] + px * (idx[1] + (py * idx[2] if mesh.dim == 3 else 0))


class PointNotInDomainError(Exception):
    """A point given to ``Function.at`` / ``gradient_at`` lies outside the mesh (Firedrake's exception of this name)."""


def _outside_unit_box(pts: np.ndarray, boxes: Sequence[int], tol: float) -> np.ndarray:
    """[m] bool: the point is outside by the evaluation kernel's own rule (pph_eval.hip), in the same arithmetic: per
    direction t = x n, c = clamp(floor(t), 0, n - 1), xi = t - c outside [-tol, 1 + tol] (NaN: outside)."""
    n = np.asarray(boxes, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        t = pts * n
        c = np.clip(np.nan_to_num(np.floor(t), nan=0.0), 0.0, n - 1.0)
        xi = t - c
        return ~np.all((xi >= -tol) & (xi <= 1.0 + tol), axis=1)


def _outside_unit_box_device(x, boxes: Sequence[int], tol: float):
    """_outside_unit_box on a device tensor of points (fp64 multiply, floor and subtraction round as the kernel's do)."""
    import torch

    n = torch.tensor(boxes, dtype=torch.float64, device=x.device)
    t = x * n
    c = torch.minimum(torch.clamp(torch.nan_to_num(torch.floor(t), nan=0.0), min=0.0), n - 1.0)
    xi = t - c
    return ~torch.all((xi >= -tol) & (xi <= 1.0 + tol), dim=1)


def point_sources(V, points, weights, tolerance: Optional[float] = None):
    """The adjoint of ``Function.at`` on the scalar or vector space ``V``: the nodal values ``b`` with
    ``b[node] = sum_m phi_node(x_m) weights[m]``, so that ``<weights, u.at(points)> = <b, u>`` for every ``u`` in ``V``
    (``pph_eval_points_adjoint``).  ``points``: ``[m, dim]``; ``weights``: ``[m]`` (``[m, ncomp]`` on a vector space).  Arrays
    give an array, CUDA tensors a tensor on the device.  Points are located by the rules of ``at``; one outside the unit
    square / cube by more than ``tolerance`` raises ``PointNotInDomainError``.  The points are taken one after the other
    (bitwise reproducible, any number per cell): the cost is linear in ``m`` - wells, not fields of points."""
    if isinstance(V, MixedFunctionSpace):
        raise ValueError("point_sources works on one scalar or vector space: use W.sub(f)")
    mesh = V.mesh()
    if mesh.distributed:
        raise NotImplementedError("point_sources is implemented for single-context meshes: build the mesh with comm=COMM_SELF")
    dim = mesh.dim
    tol = 1e-12 if tolerance is None else float(tolerance)
    if not 0.0 <= tol < 0.5:
        raise ValueError("tolerance must be in [0, 0.5) box-local units")
    ncomp = V.value_size if isinstance(V, VectorFunctionSpace) else 1
    dev = _is_tensor(points) and points.is_cuda
    if dev != (_is_tensor(weights) and weights.is_cuda):
        raise ValueError("points and weights must both be arrays or both be device tensors")
    if not dev:
        points = np.ascontiguousarray(points.detach().numpy() if _is_tensor(points) else points, dtype=np.float64)
        weights = np.ascontiguousarray(weights.detach().numpy() if _is_tensor(weights) else weights, dtype=np.float64)
    if len(points.shape) != 2 or points.shape[1] != dim:
        raise ValueError(f"points must have shape [m, {dim}], got {tuple(points.shape)}")
    m = int(points.shape[0])
    if tuple(weights.shape) not in ({(m,), (m, 1)} if ncomp == 1 else {(m, ncomp)}):
        raise ValueError(f"weights must have shape [{m}{', ' + str(ncomp) if ncomp > 1 else ''}], got {tuple(weights.shape)}")
    boxes = (mesh.nx, mesh.ny, mesh.nz)[:dim]
    if not dev:
        outside = _outside_unit_box(points, boxes, tol)
        if outside.any():
            k = int(np.argmax(outside))
            raise PointNotInDomainError(f"point {tuple(float(c) for c in points[k])} (index {k}) is outside the unit "
                                        f"{'square' if dim == 2 else 'cube'} by more than the tolerance {tol:g}")
    deg = getattr(V, "degree", 1)
    ctx = mesh.context() if deg == 1 else mesh.context(degree=deg)
    if dev:
        points, weights = points.detach().contiguous(), weights.detach().contiguous()
    out, nout = ctx.eval_points_adjoint(points, weights, None, ncomp, tol)
    if nout:
        import torch

        k = int(torch.nonzero(_outside_unit_box_device(points, boxes, tol))[0])
        raise PointNotInDomainError(f"point {tuple(points[k].tolist())} (index {k}) is outside the unit "
                                    f"{'square' if dim == 2 else 'cube'} by more than the tolerance {tol:g}")
    return out


Expr = Union[float, Constant, np.ndarray, Callable[[np.ndarray], np.ndarray], Function]


def evaluate(expr: Expr, mesh: Mesh, nodes: Optional[np.ndarray], degree: int = 1) -> np.ndarray:
    """Values of a boundary/initial datum at the LOCAL mesh vertices ``nodes`` (all local vertices if None; local =
    global on a mesh that is not distributed).  Callables see global coordinates; nodal arrays may be global (one value
    per mesh vertex) or local; Functions are read where they live.  ``degree=2``: at the nodes of the degree-2 lattice."""
    nloc = mesh.num_local_vertices() if degree == 1 else mesh.num_nodes(degree)
    count = nloc if nodes is None else len(nodes)
    if isinstance(expr, Function):
        expr = expr.vector()
        if expr.shape != (nloc,):
            raise ValueError("boundary Function must live on a scalar space of the same mesh and degree")
    if _is_tensor(expr):
        expr = expr.detach().cpu().numpy()   # (host values wanted here; DirichletBC keeps device data on the device)
    if isinstance(expr, (int, float, Constant)):
        return np.full(count, float(expr))
    if isinstance(expr, np.ndarray):
        if expr.shape == (nloc,):
            return expr if nodes is None else expr[nodes]
        if degree == 1 and expr.shape == (mesh.num_vertices(),):
            g = mesh.local_to_global(np.arange(nloc, dtype=np.int64) if nodes is None else nodes)
            return expr[g]
        raise ValueError("nodal array must have one value per mesh vertex")
    if callable(expr):
        vals = np.asarray(expr(mesh.local_node_coordinates(nodes, degree)), dtype=np.float64)
        if vals.shape != (count,):
            raise ValueError("expression must return one value per point")
        return vals
    raise TypeError(f"cannot evaluate boundary datum of type {type(expr)}")


class DirichletBC:
    """``fd.DirichletBC(W.sub(i), value, "on_boundary")``."""

    def __init__(self, V: FunctionSpace, value: Expr, sub_domain="on_boundary"):
        if sub_domain != "on_boundary":
            raise NotImplementedError('only the "on_boundary" marker is supported')
        self._V, self.value, self.sub_domain = V, value, sub_domain

    def function_space(self) -> FunctionSpace:
        return self._V

    @property
    def field(self) -> int:
        return 0 if self._V.index is None else int(self._V.index)

    def nodes_and_values(self) -> Tuple[np.ndarray, np.ndarray]:
        """LOCAL boundary nodes (this rank's slab when the mesh is distributed, ghost planes included) and their
        values.  A callable datum is evaluated once per (condition, mesh, datum version): every solve with the same
        conditions used to re-evaluate exp / sin at 394 k boundary nodes (256^3: ~20 ms per field and call).  The cache
        key holds the callable's ``version`` / ``params`` attributes when it has them (MMSPressure: its parameters), so
        a datum whose captured parameters change is evaluated again; ``invalidate()`` drops the cache for callables
        that change without saying so.  Constants, arrays and Functions are read afresh (they can be reassigned).  A CUDA
        tensor or a device-resident Function is read on the device: nodes and values are then device tensors."""
        mesh = self._V.mesh()
        deg = getattr(self._V, "degree", 1)
        dev = self._device_value(mesh)
        if dev is not None:
            nodes, nodes_dev, gnodes_dev = mesh._boundary_index(dev.device, deg)
            if dev.shape[0] == self._nloc(mesh):
                return nodes_dev, dev[nodes_dev]
            return nodes_dev, dev[gnodes_dev]
        nodes = mesh.local_boundary_nodes(deg)
        if callable(self.value) and not isinstance(self.value, (Function, Constant)):
            key = (id(mesh), id(self.value), getattr(self.value, "version", None), getattr(self.value, "params", None), deg)
            cached = getattr(self, "_cache", None)
            if cached is None or cached[0] != key:
                self._cache = (key, nodes, evaluate(self.value, mesh, nodes, deg))
            return self._cache[1], self._cache[2]
        return nodes, evaluate(self.value, mesh, nodes, deg)

    def _nloc(self, mesh) -> int:
        deg = getattr(self._V, "degree", 1)
        return mesh.num_local_vertices() if deg == 1 else mesh.num_nodes(deg)

    def _device_value(self, mesh):
        """The datum as a device tensor when it lives on the device (a CUDA tensor, a device-resident Function), else None.
        Device data stay there: nodes_and_values() then returns (int64 node tensor, value tensor) on that device."""
        v = self.value
        if isinstance(v, Function):
            if not v.on_device:
                return None
            v = v.torch()
            if v.shape[0] != self._nloc(mesh):
                raise ValueError("boundary Function must live on a scalar space of the same mesh and degree")
            return v
        if not (_is_tensor(v) and v.is_cuda):
            return None
        from . import _ffi

        _ffi.require_shared_runtime("a DirichletBC with device data")
        import torch

        nglob = mesh.num_vertices() if getattr(self._V, "degree", 1) == 1 else self._nloc(mesh)
        if v.dtype != torch.float64 or v.dim() != 1 or v.shape[0] not in (self._nloc(mesh), nglob):
            raise ValueError("nodal tensor must be 1-D float64 with one value per mesh vertex (local or global)")
        return v

    def invalidate(self) -> None:
        """Forget the evaluated datum (a callable whose captured state changed)."""
        self._cache = None
