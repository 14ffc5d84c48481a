// Degree-2 Lagrange pressures (Q2 quadrilaterals / hexahedra, P2 triangles / tetrahedra) on the structured meshes:
// lattice coordinates, cell->dof map, scalar CSR pattern and the cell-local integration of K and M.
//
// Replaces what FunctionSpace(mesh, "CG", 2) and the TSFC kernels of a degree-2 form do for the reference
// (src/perphil/forms/spaces.py:5-36, pressure_deg).  Numbering and local node order: pph_p2.h.  The Dirichlet elimination,
// lifting and monolithic fill afterwards are the generic CSR passes of pph_assemble.hip (k_lift_rhs, k_blocks,
// k_mono_*); degree 2 has no stencil-ELL storage and no multigrid hierarchy.
//
// Assembly is a row-owner gather: one lane per node walks the <= 8 boxes around it (in 3D: <= 8 boxes x 6 tetrahedra)
// in ascending cell order and adds the row of every incident cell's element matrices into its own CSR slots.  No atomics:
// the result is bitwise reproducible, and as every entry (i, j) is the sum over the same cells in the same order of
// element entries that are themselves bitwise symmetric (below), K and M come out bitwise symmetric.
//
// Element matrices: the cells are affine, so with G = |det J| J^-1 J^-T and the reference tables
//   R_ij[a][b] = int dphi_a/dxi_i dphi_b/dxi_j ,   Mref[a][b] = int phi_a phi_b      (reference cell)
// K_e[a][b] = sum_i G_ii R_ii[a][b] + sum_{i<j} G_ij (R_ij[a][b] + R_ji[a][b])  and  M_e = |det J| Mref.
// The tables are integrated once on the host, by a rule exact for the degree-4 integrands: 3 Gauss points per direction on
// [0,1]^d (Q2), the collapsed (Duffy) Gauss rule with 3 (triangles) / 4 (tetrahedra) points per direction (P2).  Per cell
// and row a lane then does DIM x DIM geometry work plus about 2 + DIM(DIM+1)/2 multiply-adds per column instead of a
// quadrature loop: the kernel is bound by the K / M traffic (16 B per entry and incident cell, L2-resident
// read-modify-write of the row's slots, 16 B per entry to HBM at the end), not by flops.
#include "pph_internal.h"
#include "pph_p2.h"
#include <cmath>

struct P2Geo {
  int kind, dim, m, cpb;   // cell kind, dimension, nodes per cell, cells per box
  int nx, ny, nzb;         // boxes per direction (nzb = 1 in 2D)
  int px, py, pz;          // lattice points per direction
};

static P2Geo p2_geo(const MeshData& mesh) {
  P2Geo g;
  g.kind = mesh.kind; g.dim = mesh.dim; g.m = p2_nodes_per_cell(mesh.kind); g.cpb = p2_cells_per_box(mesh.kind);
  g.nx = mesh.nx; g.ny = mesh.ny; g.nzb = mesh.dim == 3 ? mesh.nzl : 1;
  g.px = mesh.px; g.py = mesh.py; g.pz = mesh.pzl;
  return g;
}

// every cell holding lattice point (I,J,K), in ascending cell order: f(box id, box coords, sub-cell, local index of the point)
template <typename F>
__device__ __forceinline__ void p2_walk(const P2Geo& g, int I, int J, int K, F&& f) {
  for (int bz = (g.dim == 3 ? K / 2 - 1 : 0); bz <= (g.dim == 3 ? K / 2 : 0); ++bz) {
    if (bz < 0 || bz >= g.nzb || (g.dim == 3 && (2 * bz > K || K > 2 * bz + 2))) continue;
    for (int by = J / 2 - 1; by <= J / 2; ++by) {
      if (by < 0 || by >= g.ny || 2 * by > J || J > 2 * by + 2) continue;
      for (int bx = I / 2 - 1; bx <= I / 2; ++bx) {
        if (bx < 0 || bx >= g.nx || 2 * bx > I || I > 2 * bx + 2) continue;
        const int64_t box = bx + (int64_t)g.nx * (by + (int64_t)g.ny * bz);
        for (int s = 0; s < g.cpb; ++s) {
          for (int a = 0; a < g.m; ++a) {
            int o[3];
            p2_local_offset(g.kind, s, a, o);
            if (2 * bx + o[0] == I && 2 * by + o[1] == J && 2 * bz + o[2] == K) {
              f(box, bx, by, bz, s, a);
              break;
            }
          }
        }
      }
    }
  }
}

// columns of row (I,J,K) as bits of its 5 x 5 (x 5) window, bit (dx+2) + 5 (dy+2) + 25 (dz+2): ascending bits = ascending
// columns (every column lies inside the box of lattice points, whose x extent is narrower than one y step)
struct P2Mask {
  unsigned long long w[2];
  __device__ void set(int b) { w[b >> 6] |= 1ull << (b & 63); }
  __device__ bool has(int b) const { return (w[b >> 6] >> (b & 63)) & 1ull; }
  __device__ int below(int b) const {   // set bits below b
    if (b < 64) return __popcll(w[0] & ((1ull << b) - 1ull));
    return __popcll(w[0]) + __popcll(w[1] & ((1ull << (b - 64)) - 1ull));
  }
  __device__ int count() const { return __popcll(w[0]) + __popcll(w[1]); }
};

__device__ __forceinline__ void p2_ijk(const P2Geo& g, int64_t id, int* I, int* J, int* K) {
  *I = (int)(id % g.px);
  const int64_t t = id / g.px;
  *J = (int)(t % g.py);
  *K = (int)(t / g.py);
}

__device__ __forceinline__ P2Mask p2_row_mask(const P2Geo& g, int I, int J, int K) {
  P2Mask mk;
  mk.w[0] = mk.w[1] = 0ull;
  p2_walk(g, I, J, K, [&](int64_t, int bx, int by, int bz, int s, int) {
    for (int b = 0; b < g.m; ++b) {
      int o[3];
      p2_local_offset(g.kind, s, b, o);
      mk.set((2 * bx + o[0] - I + 2) + 5 * (2 * by + o[1] - J + 2) + 25 * (2 * bz + o[2] - K + 2));
    }
  });
  return mk;
}

// ------------------------------------------------------------------------------------------------
// lattice coordinates, cell->dof map, pattern
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_p2_coords(double* __restrict__ cx, double* __restrict__ cy, double* __restrict__ cz,
                                                   P2Geo g, int64_t n, double sx, double sy, double sz) {
  for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < n; id += (int64_t)gridDim.x * blockDim.x) {
    int I, J, K;
    p2_ijk(g, id, &I, &J, &K);
    cx[id] = (double)I / sx;
    cy[id] = (double)J / sy;
    if (g.dim == 3) cz[id] = (double)K / sz;
  }
}

__global__ __launch_bounds__(256) void k_p2_dofmap(int32_t* __restrict__ cells, P2Geo g, int64_t nbox) {
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < nbox; b += (int64_t)gridDim.x * blockDim.x) {
    const int bx = (int)(b % g.nx);
    const int64_t t = b / g.nx;
    const int by = (int)(t % g.ny), bz = (int)(t / g.ny);
    for (int s = 0; s < g.cpb; ++s) {
      int32_t* c = cells + (b * g.cpb + s) * g.m;
      for (int a = 0; a < g.m; ++a) {
        int o[3];
        p2_local_offset(g.kind, s, a, o);
        c[a] = (int32_t)((2 * bx + o[0]) + (int64_t)g.px * ((2 * by + o[1]) + (int64_t)g.py * (2 * bz + o[2])));
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_p2_row_count(int32_t* __restrict__ cnt, P2Geo g, int64_t n) {
  for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < n; id += (int64_t)gridDim.x * blockDim.x) {
    int I, J, K;
    p2_ijk(g, id, &I, &J, &K);
    cnt[id] = p2_row_mask(g, I, J, K).count();
  }
}

__global__ __launch_bounds__(256) void k_p2_row_fill(int32_t* __restrict__ col, const int64_t* __restrict__ rowptr, P2Geo g,
                                                     int64_t n) {
  for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < n; id += (int64_t)gridDim.x * blockDim.x) {
    int I, J, K;
    p2_ijk(g, id, &I, &J, &K);
    const P2Mask mk = p2_row_mask(g, I, J, K);
    int64_t o = rowptr[id];
    for (int w = 0; w < 125; ++w)
      if (mk.has(w)) {
        const int dx = w % 5 - 2, dy = (w / 5) % 5 - 2, dz = w / 25 - 2;
        col[o++] = (int32_t)((I + dx) + (int64_t)g.px * ((J + dy) + (int64_t)g.py * (K + dz)));
      }
  }
}

// longest row of the pattern (one block)
__global__ __launch_bounds__(256) void k_p2_max_row(const int64_t* __restrict__ rowptr, int64_t n, int* __restrict__ out) {
  __shared__ int lds[256];
  int mx = 0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const int len = (int)(rowptr[i + 1] - rowptr[i]);
    mx = len > mx ? len : mx;
  }
  lds[threadIdx.x] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o && lds[threadIdx.x + o] > lds[threadIdx.x]) lds[threadIdx.x] = lds[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = lds[0];
}

static int p2_grid(int64_t n) {
  int64_t b = ceil_div64(n, 256);
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// degree-2 sizes, coordinates, cell->dof map and scalar CSR pattern of `mesh` (whole mesh, one context)
int pph_p2_mesh(pph_ctx* ctx, MeshData& mesh) {
  PPH_REQUIRE(ctx, mesh.z0 == 0 && mesh.glo == 0 && mesh.ghi == 0 && (mesh.dim == 2 || mesh.nzl == mesh.nz),
              "degree-2 meshes are whole meshes (no slab decomposition)");
  mesh.m = p2_nodes_per_cell(mesh.kind);
  mesh.px = 2 * mesh.nx + 1;
  mesh.py = 2 * mesh.ny + 1;
  mesh.pzl = (mesh.dim == 3) ? 2 * mesh.nzl + 1 : 1;
  mesh.n = (int64_t)mesh.px * mesh.py * mesh.pzl;
  const int64_t nbox = (int64_t)mesh.nx * mesh.ny * (mesh.dim == 3 ? mesh.nzl : 1);
  mesh.ncell = nbox * p2_cells_per_box(mesh.kind);
  PPH_REQUIRE(ctx, mesh.n < (int64_t)1073741823, "mesh has %lld degree-2 nodes per field: beyond the int32 dof range",
              (long long)mesh.n);
  mesh.all_affine = false;   // (the multilinear kernels' flags: unused at degree 2)
  mesh.uniform = false;
  const P2Geo g = p2_geo(mesh);
  const int64_t n = mesh.n;
  PPH_TRY(mesh.cx.alloc(ctx, (size_t)n));
  PPH_TRY(mesh.cy.alloc(ctx, (size_t)n));
  PPH_TRY(mesh.cz.alloc(ctx, mesh.dim == 3 ? (size_t)n : 1));
  PPH_TRY(mesh.cells.alloc(ctx, (size_t)mesh.ncell * mesh.m));
  hipLaunchKernelGGL(k_p2_coords, dim3(p2_grid(n)), dim3(256), 0, ctx->stream, mesh.cx.p, mesh.cy.p, mesh.cz.p, g, n,
                     2.0 * mesh.nx, 2.0 * mesh.ny, 2.0 * (mesh.nz > 0 ? mesh.nz : 1));
  hipLaunchKernelGGL(k_p2_dofmap, dim3(p2_grid(nbox)), dim3(256), 0, ctx->stream, mesh.cells.p, g, nbox);
  // the pattern (built here: every degree-2 operator is CSR)
  DevBuf<int32_t> cnt;
  PPH_TRY(cnt.alloc(ctx, (size_t)n));
  hipLaunchKernelGGL(k_p2_row_count, dim3(p2_grid(n)), dim3(256), 0, ctx->stream, cnt.p, g, n);
  int64_t nnz = 0;
  const int scanned = pph_scan_counts(ctx, cnt.p, n, mesh.rowptr, &nnz);
  cnt.release();   // (before the size check, so that a refused mesh does not leak it)
  PPH_TRY(scanned);
  PPH_REQUIRE(ctx, nnz > 0 && nnz < (int64_t)2147483647, "degree-2 scalar block of %lld entries: beyond the int32 positions of "
              "the CSR pattern", (long long)nnz);
  PPH_TRY(mesh.col.alloc(ctx, (size_t)nnz));
  hipLaunchKernelGGL(k_p2_row_fill, dim3(p2_grid(n)), dim3(256), 0, ctx->stream, mesh.col.p, mesh.rowptr.p, g, n);
  DevBuf<int> mx;
  PPH_TRY(mx.alloc(ctx, 1));
  hipLaunchKernelGGL(k_p2_max_row, dim3(1), dim3(256), 0, ctx->stream, mesh.rowptr.p, n, mx.p);
  int h = 0;
  PPH_HIP(ctx, hipMemcpyAsync(&h, mx.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  PPH_HIP(ctx, hipGetLastError());
  mx.release();
  mesh.max_row = h;
  mesh.nnzb = nnz;
  mesh.pattern_ok = true;
  return PPH_OK;
}

// ------------------------------------------------------------------------------------------------
// reference tables (host) and the row-owner assembly of K and M
// ------------------------------------------------------------------------------------------------
static void p2_gauss01(int nq, double* x, double* w) {   // Gauss-Legendre on [0,1]
  const double PI = 3.14159265358979323846;
  for (int i = 0; i < nq; ++i) {
    double z = std::cos(PI * (i + 0.75) / (nq + 0.5)), dp = 1.0;
    for (int it = 0; it < 100; ++it) {
      double p0 = 1.0, p1 = 0.0;
      for (int k = 1; k <= nq; ++k) { const double p2 = p1; p1 = p0; p0 = ((2.0 * k - 1.0) * z * p1 - (k - 1.0) * p2) / k; }
      dp = nq * (z * p0 - p1) / (z * z - 1.0);
      const double dz = p0 / dp;
      z -= dz;
      if (std::fabs(dz) < 1e-17) break;
    }
    x[i] = 0.5 * (1.0 - z);
    w[i] = 1.0 / ((1.0 - z * z) * dp * dp);
  }
}

template <int KIND>
static void p2_tables_t(std::vector<double>& tab) {
  constexpr int D = (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_TRI) ? 2 : 3;
  constexpr bool simplex = (KIND == PPH_CELL_TRI || KIND == PPH_CELL_TET);
  const int m = p2_nodes_per_cell(KIND), mm = m * m;
  const int nq = simplex ? (D == 2 ? 3 : 4) : 3;
  double gx[8], gw[8];
  p2_gauss01(nq, gx, gw);
  tab.assign((size_t)(D * D + 1) * mm, 0.0);   // [i*D + j][a][b] then Mref[a][b]
  const int npts = D == 2 ? nq * nq : nq * nq * nq;
  for (int q = 0; q < npts; ++q) {
    const int qi[3] = {q % nq, (q / nq) % nq, q / (nq * nq)};
    double xi[3], w;
    if (!simplex) {
      w = 1.0;
      for (int e = 0; e < D; ++e) { xi[e] = gx[qi[e]]; w *= gw[qi[e]]; }
    } else {   // collapsed rule (pph_post.hip): xi_1 = u, xi_2 = v (1 - u), xi_3 = t (1 - u)(1 - v)
      const double u = gx[qi[0]], v = gx[qi[1]];
      xi[0] = u; xi[1] = v * (1.0 - u);
      w = gw[qi[0]] * gw[qi[1]] * (1.0 - u);
      if (D == 3) { const double t = gx[qi[2]]; xi[2] = t * (1.0 - u) * (1.0 - v); w *= gw[qi[2]] * (1.0 - u) * (1.0 - v); }
    }
    double N[PPH_P2_MAXM], dN[PPH_P2_MAXM][3];
    for (int a = 0; a < m; ++a) p2_basis<KIND>(a, xi, &N[a], dN[a]);
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b) {
        for (int i = 0; i < D; ++i)
          for (int j = 0; j < D; ++j) tab[(size_t)(i * D + j) * mm + a * m + b] += w * (dN[a][i] * dN[b][j]);
        tab[(size_t)D * D * mm + a * m + b] += w * (N[a] * N[b]);
      }
  }
  // the exact tables are rationals whose smallest non-zero magnitude is ~1e-3 of the largest of the same table; what the
  // quadrature leaves of an exact zero (~1e-17) would otherwise reach K / M as an entry of the size of a rounding error
  // of the whole element matrix, where the exact entry is 0
  for (int t = 0; t <= D * D; ++t) {
    double mx = 0.0;
    for (int k = 0; k < mm; ++k) mx = std::fmax(mx, std::fabs(tab[(size_t)t * mm + k]));
    for (int k = 0; k < mm; ++k)
      if (std::fabs(tab[(size_t)t * mm + k]) <= 1e-12 * mx) tab[(size_t)t * mm + k] = 0.0;
  }
}

void pph_p2_tables(int kind, std::vector<double>& tab) {
  if (kind == PPH_CELL_QUAD) p2_tables_t<PPH_CELL_QUAD>(tab);
  else if (kind == PPH_CELL_TRI) p2_tables_t<PPH_CELL_TRI>(tab);
  else if (kind == PPH_CELL_HEX) p2_tables_t<PPH_CELL_HEX>(tab);
  else p2_tables_t<PPH_CELL_TET>(tab);
}

// affine frame of a cell: G = |det J| J^-1 J^-T (symmetric) and |det J|
template <int D>
__device__ __forceinline__ void p2_frame(const double X[D + 1][3], double G[D][D], double* adet) {
  double J[D][D];   // J[d][e] = X_{e+1}[d] - X_0[d]
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int e = 0; e < D; ++e) J[d][e] = X[e + 1][d] - X[0][d];
  double Ji[D][D], det;
  if constexpr (D == 2) {
    det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double r = 1.0 / det;
    Ji[0][0] = J[1][1] * r;  Ji[0][1] = -J[0][1] * r;
    Ji[1][0] = -J[1][0] * r; Ji[1][1] = J[0][0] * r;
  } else {
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    const double r = 1.0 / det;
    Ji[0][0] = c00 * r;
    Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r;
    Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r;
    Ji[1][0] = c01 * r;
    Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r;
    Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r;
    Ji[2][0] = c02 * r;
    Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r;
    Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r;
  }
  *adet = fabs(det);
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) s += Ji[i][k] * Ji[j][k];
      G[i][j] = *adet * s;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_p2_km(double sx, double sy, double sz, const int64_t* __restrict__ rowptr,
                                               const double* __restrict__ tab, P2Geo g, int64_t n, double* __restrict__ K,
                                               double* __restrict__ M) {
  constexpr int D = (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_TRI) ? 2 : 3;
  constexpr int m = (KIND == PPH_CELL_QUAD) ? 9 : (KIND == PPH_CELL_TRI) ? 6 : (KIND == PPH_CELL_HEX) ? 27 : 10;
  constexpr int mm = m * m;
  const double* Mref = tab + D * D * mm;
  for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
    int I, J, Kk;
    p2_ijk(g, row, &I, &J, &Kk);
    const P2Mask mk = p2_row_mask(g, I, J, Kk);
    const int64_t base = rowptr[row], len = rowptr[row + 1] - base;
    for (int64_t k = 0; k < len; ++k) { K[base + k] = 0.0; M[base + k] = 0.0; }
    p2_walk(g, I, J, Kk, [&](int64_t, int bx, int by, int bz, int s, int a) {
      // the frame relative to the box: lattice offsets / lattice points per unit length.  The differences of the cell's
      // absolute coordinates (k_p2_coords: I / sx) would carry their rounding, ~u |x|, into J = O(h): a relative error
      // ~u / h that grows with the mesh; these are exact up to one rounding, the same in every box
      double X[D + 1][3];
#pragma unroll
      for (int r = 0; r <= D; ++r) {
        int o[3];
        p2_local_offset(KIND, s, p2_frame_node(KIND, r), o);
        X[r][0] = (double)o[0] / sx;
        X[r][1] = (double)o[1] / sy;
        X[r][2] = (D == 3) ? (double)o[2] / sz : 0.0;
      }
      double G[D][D], adet;
      p2_frame<D>(X, G, &adet);
      for (int b = 0; b < m; ++b) {
        int o[3];
        p2_local_offset(KIND, s, b, o);
        const int w = (2 * bx + o[0] - I + 2) + 5 * (2 * by + o[1] - J + 2) + 25 * (2 * bz + o[2] - Kk + 2);
        const int64_t pos = base + mk.below(w);
        const int ab = a * m + b;
        double kv = 0.0, ka = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
          const double t = G[i][i] * tab[(i * D + i) * mm + ab];
          kv += t;
          ka += fabs(t);
        }
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
          for (int j = i + 1; j < D; ++j) {
            const double t = G[i][j] * (tab[(i * D + j) * mm + ab] + tab[(j * D + i) * mm + ab]);
            kv += t;
            ka += fabs(t);
          }
        // an entry that cancels to exactly 0 (e.g. right simplices) leaves ~u of its terms: below its own rounding bound
        // it is 0 (the non-zero entries of these cells are far above it)
        if (fabs(kv) <= 16.0 * 1.1102230246251565e-16 * ka) kv = 0.0;
        K[pos] += kv;
        M[pos] += adet * Mref[ab];
      }
    });
  }
}

int pph_p2_assemble_KM(pph_ctx* ctx, MeshData& mesh) {
  PPH_REQUIRE(ctx, mesh.degree == 2 && mesh.pattern_ok, "degree-2 assembly without a degree-2 mesh");
  PPH_TRY(mesh.K.alloc(ctx, (size_t)mesh.nnzb));
  PPH_TRY(mesh.M.alloc(ctx, (size_t)mesh.nnzb));
  std::vector<double> tab;
  pph_p2_tables(mesh.kind, tab);
  DevBuf<double> dt;
  PPH_TRY(dt.alloc(ctx, tab.size()));
  PPH_HIP(ctx, hipMemcpyAsync(dt.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
  const P2Geo g = p2_geo(mesh);
  const int grid = p2_grid(mesh.n);
#define PPH_P2_KM(KD)                                                                                                  \
  hipLaunchKernelGGL(k_p2_km<KD>, dim3(grid), dim3(256), 0, ctx->stream, 2.0 * mesh.nx, 2.0 * mesh.ny,               \
                     2.0 * (mesh.nz > 0 ? mesh.nz : 1), mesh.rowptr.p, dt.p, g, mesh.n, mesh.K.p, mesh.M.p)
  if (mesh.kind == PPH_CELL_QUAD) PPH_P2_KM(PPH_CELL_QUAD);
  else if (mesh.kind == PPH_CELL_TRI) PPH_P2_KM(PPH_CELL_TRI);
  else if (mesh.kind == PPH_CELL_HEX) PPH_P2_KM(PPH_CELL_HEX);
  else PPH_P2_KM(PPH_CELL_TET);
#undef PPH_P2_KM
  PPH_HIP(ctx, hipGetLastError());
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the table buffer is freed below)
  dt.release();
  return PPH_OK;
}

// rownear (pph_assemble.hip: k_row_near) from the CSR pattern: the degree-2 rows reach 2 lattice steps
__global__ __launch_bounds__(256) void k_p2_row_near(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                     const uint8_t* __restrict__ m1, const uint8_t* __restrict__ m2, int64_t n,
                                                     uint8_t* __restrict__ rownear) {
  for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
    int f = (m1[row] | m2[row]) != 0;
    for (int64_t k = rowptr[row]; k < rowptr[row + 1]; ++k) {
      const int32_t c = col[k];
      f |= ((m1[c] | m2[c]) & 1) != 0;
    }
    rownear[row] = (uint8_t)f;
  }
}

void pph_p2_row_near(pph_ctx* ctx, const MeshData& mesh, const uint8_t* m1, const uint8_t* m2, uint8_t* out) {
  hipLaunchKernelGGL(k_p2_row_near, dim3(p2_grid(mesh.n)), dim3(256), 0, ctx->stream, mesh.rowptr.p, mesh.col.p, m1, m2,
                     mesh.n, out);
}
