// Mass balance: boundary fluxes, volume integrals and consistent nodal fluxes of finite-element pressures.
//
// No reference counterpart computes these; they stand beside calculate_darcy_velocity_from_pressure (reference
// src/perphil/utils/postprocessing.py:34-63: the same -k grad p_h, there projected) and the model's mass transfer term
// xi = beta/mu (p1 - p2) (src/perphil/forms/dpp.py:27).  CG-1 and degree-2 (pph_p2.h) fields on all four cell kinds, whole
// meshes on a single context.
//
//   k_face_flux     F_s = int_{side s} -kappa grad p_h . n ds for the 2 dim sides of the unit box (1: x = 0, 2: x = 1, 3: y = 0,
//                   4: y = 1, 5: z = 0, 6: z = 1), gradient of the cell that owns the facet, outward axis normal.  One thread per
//                   (side, box of the boundary layer): the launch grows with the boundary, not with the mesh.
//   k_integrate     int p_h dx, one thread per box.
//   k_dpp_nodal_flux r1 = a K p1 + b M (p1 - p2), r2 = c K p2 - b M (p1 - p2) on the un-eliminated CSR operators K and M
//                   (a = k1/mu, b = beta/mu, c = k2/mu): minus the outward flux of each network weighted with phi_i.
//
// The meshes are uniform boxes (pph_mesh.hip: node i at i / n), so the geometry is arithmetic, as in pph_eval.hip: a gradient
// is the box-local one times n_e, a box face has area prod_{f != d} 1 / n_f.  No quadrature: every integral below is the
// closed form of the integral of the basis itself, exact for the finite-element function.
//   Q1 / Q2 (per direction, nodes at 0, 1 or 0, 1/2, 1): int N_i = (1/2, 1/2) or Simpson's (1/6, 2/3, 1/6);
//     N_i'(0) = (-1, 1) or (-3, 4, -1), N_i'(1) = (-1, 1) or (1, -4, 3).  The normal derivative integrated over a face is the
//     tensor product of the derivative weights along the normal and the integral weights along the tangents.
//   P1 / P2: every sub-cell of a box (left-diagonal triangles, Kuhn tetrahedra) has exactly one edge along each axis.  A sub-cell
//     has a facet on side (d, hi) when all its vertices but one (`o`) lie there; its edge along d then joins o and a facet
//     vertex, and d/dxi_d is the derivative along that edge: u(end) - u(start) for P1, and for P2, whose gradient is linear, the
//     edge derivative at the facet's centroid times the facet's share of the box face (1, or 1/2 for the two triangles of a Kuhn
//     box face).  int N_a over a cell: P1 |c| / (dim + 1); P2 triangle 0 (vertices), |c| / 3 (edges); P2 tetrahedron -|c| / 20,
//     |c| / 5.
//
// Determinism: no floating-point atomics.  A thread adds its items in grid-stride order, a workgroup adds its threads in a
// fixed LDS tree, k_flux_sum adds the workgroups' partial sums in a fixed order; the grid is a function of the mesh alone.
// Two calls give the same bits.
#include "pph_internal.h"
#include "pph_p2.h"

#define FLUX_MAX_BLOCKS 2048   // partial sums per quantity

// sum over the workgroup (256 threads), fixed order; every thread gets it
__device__ static inline double flux_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// out[q] = sum of part[q * FLUX_MAX_BLOCKS + i], i < nblocks; one workgroup per quantity q
__global__ __launch_bounds__(256) void k_flux_sum(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  __shared__ double lds[256];
  const double* p = part + (int64_t)blockIdx.x * FLUX_MAX_BLOCKS;
  double v = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) v += p[i];
  v = flux_block_sum(v, lds);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

template <int KIND, int DEG>
struct FluxCell {
  static constexpr int DIM = (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_TRI) ? 2 : 3;
  static constexpr bool SIMPLEX = (KIND == PPH_CELL_TRI || KIND == PPH_CELL_TET);
  static constexpr int NB = (DEG == 2) ? ((KIND == PPH_CELL_QUAD) ? 9 : (KIND == PPH_CELL_TRI) ? 6 : (KIND == PPH_CELL_HEX) ? 27 : 10)
                                       : (SIMPLEX ? DIM + 1 : (1 << DIM));
  static constexpr int CPB = (KIND == PPH_CELL_TRI) ? 2 : (KIND == PPH_CELL_TET) ? 6 : 1;   // cells per box
};

// per-direction weights of the tensor-product elements: integral of node i's basis over [0, 1], its derivative at t = hi
template <int DEG>
__device__ static inline double flux_w_int(int i) {
  if constexpr (DEG == 1) return 0.5;
  else return i == 1 ? 2.0 / 3.0 : 1.0 / 6.0;
}
template <int DEG>
__device__ static inline double flux_w_der(int i, int hi) {
  if constexpr (DEG == 1) return i ? 1.0 : -1.0;
  else return hi ? (i == 0 ? 1.0 : (i == 1 ? -4.0 : 3.0)) : (i == 0 ? -3.0 : (i == 1 ? 4.0 : -1.0));
}

struct FluxGeo {
  int n[3];         // boxes per direction (2D: n[2] = 1)
  int64_t off[7];   // off[s]: first item of side s + 1 in the list of (side, box) pairs; off[2 dim]: their number
};

// the integral over the face (d, hi) of the unit box of d p_h / d xi_d (box-local units), from the cells of `box` that have a
// facet there
template <int KIND, int DEG>
__device__ static inline double flux_box_face(const int32_t* __restrict__ cells, const double* __restrict__ u, int64_t box,
                                              int d, int hi) {
  using C = FluxCell<KIND, DEG>;
  constexpr int DIM = C::DIM, NB = C::NB;
  double acc = 0.0;
  if constexpr (!C::SIMPLEX) {
    const int32_t* cn = cells + box * NB;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int ib[3] = {b % (DEG + 1), (b / (DEG + 1)) % (DEG + 1), b / ((DEG + 1) * (DEG + 1))};
      double w = 1.0;
#pragma unroll
      for (int e = 0; e < DIM; ++e) w *= (e == d) ? flux_w_der<DEG>(ib[e], hi) : flux_w_int<DEG>(ib[e]);
      acc += w * u[cn[b]];
    }
  } else {
#pragma unroll
    for (int sub = 0; sub < C::CPB; ++sub) {
      // the vertex off the side (`o`), or no facet there; the ends (lo -> up) of the cell's edge along d
      int on = 0, o = 0, lo = 0, up = 0;
#pragma unroll
      for (int r = 0; r <= DIM; ++r) {
        const int v = p2_simplex_vertex(KIND, sub, r);
        if (((v >> d) & 1) == hi) ++on; else o = r;
      }
      if (on != DIM) continue;
      const int vo = p2_simplex_vertex(KIND, sub, o);
#pragma unroll
      for (int r = 0; r <= DIM; ++r)
        if (p2_simplex_vertex(KIND, sub, r) == (vo ^ (1 << d))) { lo = hi ? o : r; up = hi ? r : o; }
      const int32_t* cn = cells + (box * C::CPB + sub) * NB;
      double der = 0.0;
      if constexpr (DEG == 1) {
#pragma unroll
        for (int r = 0; r <= DIM; ++r) der += (r == up ? 1.0 : (r == lo ? -1.0 : 0.0)) * u[cn[r]];
      } else {
        double xr[DIM];   // reference coordinates of pph_p2.h (xr_j = lambda_{j+1}) of the facet's centroid
#pragma unroll
        for (int j = 0; j < DIM; ++j) xr[j] = (j + 1 == o) ? 0.0 : 1.0 / (double)DIM;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          double nv, dn[3];
          p2_basis<KIND>(b, xr, &nv, dn);
          double along = 0.0;   // reference vertex r > 0 is e_{r-1}, vertex 0 the origin
#pragma unroll
          for (int j = 0; j < DIM; ++j) along += (j + 1 == up ? dn[j] : 0.0) - (j + 1 == lo ? dn[j] : 0.0);
          der += along * u[cn[b]];
        }
      }
      acc += der * (DIM == 3 ? 0.5 : 1.0);
    }
  }
  return acc;
}

// part[s * FLUX_MAX_BLOCKS + block]: this workgroup's share of F_{s+1}
template <int KIND, int DEG>
__global__ __launch_bounds__(256) void k_face_flux(const int32_t* __restrict__ cells, const double* __restrict__ u, FluxGeo g,
                                                   double kappa, double* __restrict__ part) {
  constexpr int DIM = FluxCell<KIND, DEG>::DIM;
  __shared__ double lds[256];
  double acc[2 * DIM];
#pragma unroll
  for (int s = 0; s < 2 * DIM; ++s) acc[s] = 0.0;
  const int64_t total = g.off[2 * DIM];
  for (int64_t it = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
    int s = 0;
#pragma unroll
    for (int q = 1; q < 2 * DIM; ++q) s += (it >= g.off[q]) ? 1 : 0;
    const int d = s >> 1, hi = s & 1;
    // the box: position hi ? n_d - 1 : 0 along d, the item's index over the other directions in ascending order
    int64_t f = it - g.off[s], box = 0, stride = 1;
    double scale = (double)g.n[d];   // d/dx_d = n_d d/dxi_d ...
#pragma unroll
    for (int e = 0; e < DIM; ++e) {
      int c;
      if (e == d) c = hi ? g.n[e] - 1 : 0;
      else { c = (int)(f % g.n[e]); f /= g.n[e]; scale /= (double)g.n[e]; }   // ... times the face's area
      box += stride * c;
      stride *= g.n[e];
    }
    const double v = flux_box_face<KIND, DEG>(cells, u, box, d, hi) * scale * (hi ? -kappa : kappa);
#pragma unroll
    for (int q = 0; q < 2 * DIM; ++q) acc[q] += (q == s) ? v : 0.0;
  }
#pragma unroll
  for (int q = 0; q < 2 * DIM; ++q) {
    const double t = flux_block_sum(acc[q], lds);
    if (threadIdx.x == 0) part[(int64_t)q * FLUX_MAX_BLOCKS + blockIdx.x] = t;
  }
}

// part[block]: this workgroup's share of int p_h dx / |box|
template <int KIND, int DEG>
__global__ __launch_bounds__(256) void k_integrate(const int32_t* __restrict__ cells, const double* __restrict__ u, int64_t nbox,
                                                   double* __restrict__ part) {
  using C = FluxCell<KIND, DEG>;
  constexpr int DIM = C::DIM, NB = C::NB;
  __shared__ double lds[256];
  double acc = 0.0;
  for (int64_t box = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; box < nbox; box += (int64_t)gridDim.x * blockDim.x) {
    double sb = 0.0;
#pragma unroll
    for (int sub = 0; sub < C::CPB; ++sub) {
      const int32_t* cn = cells + (box * C::CPB + sub) * NB;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        double w;
        if constexpr (!C::SIMPLEX) {
          const int ib[3] = {b % (DEG + 1), (b / (DEG + 1)) % (DEG + 1), b / ((DEG + 1) * (DEG + 1))};
          w = 1.0;
#pragma unroll
          for (int e = 0; e < DIM; ++e) w *= flux_w_int<DEG>(ib[e]);
        } else if constexpr (DEG == 1) {
          w = 1.0 / (double)(DIM + 1);
        } else if constexpr (DIM == 2) {
          w = b < 3 ? 0.0 : 1.0 / 3.0;
        } else {
          w = b < 4 ? -1.0 / 20.0 : 1.0 / 5.0;
        }
        if (w != 0.0) sb += w * u[cn[b]];
      }
    }
    acc += sb / (double)C::CPB;
  }
  const double t = flux_block_sum(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// 8 lanes per row of the scalar CSR pattern; p and r field-major (2 n)
__global__ __launch_bounds__(256) void k_dpp_nodal_flux(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const double* __restrict__ K, const double* __restrict__ M,
                                                        const double* __restrict__ p, int64_t n, double a, double b, double c,
                                                        double* __restrict__ r) {
  const int lane = threadIdx.x & 7;
  for (int64_t base = (int64_t)blockIdx.x * 32; base < n; base += (int64_t)gridDim.x * 32) {   // (uniform over the workgroup)
    const int64_t row = base + (threadIdx.x >> 3);
    double s1 = 0.0, s2 = 0.0, sm = 0.0;
    if (row < n) {
      const int64_t end = rowptr[row + 1];
      for (int64_t j = rowptr[row] + lane; j < end; j += 8) {
        const int32_t cj = col[j];
        const double p1 = p[cj], p2 = p[n + cj], k = K[j];
        s1 += k * p1;
        s2 += k * p2;
        sm += M[j] * (p1 - p2);
      }
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o, 64);
      s2 += __shfl_xor(s2, o, 64);
      sm += __shfl_xor(sm, o, 64);
    }
    if (row < n && lane == 0) {
      r[row] = a * s1 + b * sm;
      r[n + row] = c * s2 - b * sm;
    }
  }
}

static int flux_check(pph_ctx* ctx, const char* who, bool buffers) {
  PPH_REQUIRE(ctx, ctx->mesh_ok, "%s before pph_mesh_build", who);
  PPH_REQUIRE(ctx, ctx->world == 1, "%s is implemented for single-context meshes", who);
  PPH_REQUIRE(ctx, buffers, "%s: NULL buffer", who);
  return PPH_OK;
}

static int flux_grid(int64_t items) {
  const int64_t nb = ceil_div64(items, 256);
  return (int)(nb < 1 ? 1 : (nb < FLUX_MAX_BLOCKS ? nb : FLUX_MAX_BLOCKS));
}

template <int KIND>
static void flux_launch(pph_ctx* ctx, int degree, int grid, const double* u, const FluxGeo& g, double kappa, double* part) {
  const int32_t* cells = ctx->mesh.cells.p;
  if (degree == 2) hipLaunchKernelGGL((k_face_flux<KIND, 2>), dim3(grid), dim3(256), 0, ctx->stream, cells, u, g, kappa, part);
  else hipLaunchKernelGGL((k_face_flux<KIND, 1>), dim3(grid), dim3(256), 0, ctx->stream, cells, u, g, kappa, part);
}

template <int KIND>
static void integrate_launch(pph_ctx* ctx, int degree, int grid, const double* u, int64_t nbox, double* part) {
  const int32_t* cells = ctx->mesh.cells.p;
  if (degree == 2) hipLaunchKernelGGL((k_integrate<KIND, 2>), dim3(grid), dim3(256), 0, ctx->stream, cells, u, nbox, part);
  else hipLaunchKernelGGL((k_integrate<KIND, 1>), dim3(grid), dim3(256), 0, ctx->stream, cells, u, nbox, part);
}

// the results of the two reductions reach the host through `part` (released by the entry point whichever way the call ends)
static int boundary_flux_dev(pph_ctx* ctx, DevBuf<double>& part, const double* u, double kappa, double* out6) {
  const MeshData& m = ctx->mesh;
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  FluxGeo g;
  g.n[0] = m.nx; g.n[1] = m.ny; g.n[2] = (m.dim == 3) ? m.nzl : 1;
  g.off[0] = 0;
  for (int s = 0; s < 6; ++s) {
    int64_t cnt = 0;
    if (s < 2 * m.dim) {
      cnt = 1;
      for (int e = 0; e < m.dim; ++e) if (e != s / 2) cnt *= g.n[e];
    }
    g.off[s + 1] = g.off[s] + cnt;
  }
  const int nside = 2 * m.dim;
  PPH_TRY(part.alloc(ctx, (size_t)6 * FLUX_MAX_BLOCKS + 6));
  double* res = part.p + (size_t)6 * FLUX_MAX_BLOCKS;
  const int grid = flux_grid(g.off[nside]);
  if (m.kind == PPH_CELL_QUAD) flux_launch<PPH_CELL_QUAD>(ctx, m.degree, grid, u, g, kappa, part.p);
  else if (m.kind == PPH_CELL_TRI) flux_launch<PPH_CELL_TRI>(ctx, m.degree, grid, u, g, kappa, part.p);
  else if (m.kind == PPH_CELL_HEX) flux_launch<PPH_CELL_HEX>(ctx, m.degree, grid, u, g, kappa, part.p);
  else flux_launch<PPH_CELL_TET>(ctx, m.degree, grid, u, g, kappa, part.p);
  hipLaunchKernelGGL(k_flux_sum, dim3(nside), dim3(256), 0, ctx->stream, part.p, grid, res);
  PPH_HIP(ctx, hipGetLastError());
  for (int s = 0; s < 6; ++s) out6[s] = 0.0;
  PPH_HIP(ctx, hipMemcpyAsync(out6, res, sizeof(double) * nside, hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PPH_OK;
}

static int integrate_dev(pph_ctx* ctx, DevBuf<double>& part, const double* u, double* out1) {
  const MeshData& m = ctx->mesh;
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t nbox = (int64_t)m.nx * m.ny * (m.dim == 3 ? m.nzl : 1);
  PPH_TRY(part.alloc(ctx, (size_t)FLUX_MAX_BLOCKS + 1));
  double* res = part.p + FLUX_MAX_BLOCKS;
  const int grid = flux_grid(nbox);
  if (m.kind == PPH_CELL_QUAD) integrate_launch<PPH_CELL_QUAD>(ctx, m.degree, grid, u, nbox, part.p);
  else if (m.kind == PPH_CELL_TRI) integrate_launch<PPH_CELL_TRI>(ctx, m.degree, grid, u, nbox, part.p);
  else if (m.kind == PPH_CELL_HEX) integrate_launch<PPH_CELL_HEX>(ctx, m.degree, grid, u, nbox, part.p);
  else integrate_launch<PPH_CELL_TET>(ctx, m.degree, grid, u, nbox, part.p);
  hipLaunchKernelGGL(k_flux_sum, dim3(1), dim3(256), 0, ctx->stream, part.p, grid, res);
  PPH_HIP(ctx, hipGetLastError());
  double sum = 0.0;
  PPH_HIP(ctx, hipMemcpyAsync(&sum, res, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *out1 = sum / (double)nbox;   // (|box| = 1 / nbox)
  return PPH_OK;
}

// K and M of the mesh (integrated on demand, kept by the mesh like the Darcy projection's) and the product kernel, enqueued on
// the context stream (also the CSR formulation of pph_transient.hip's step right-hand side)
int pph_nodal_flux_launch(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p, double* r) {
  MeshData& m = ctx->mesh;
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  if (!m.km_valid) {
    PPH_TRY(pph_launch_assemble_KM(ctx, m));
    m.km_valid = true;
  }
  PPH_TRY(pph_ensure_pattern(ctx, m));
  const int64_t nb = ceil_div64(m.n, 32);
  const int grid = (int)(nb < 65536 ? nb : 65536);
  hipLaunchKernelGGL(k_dpp_nodal_flux, dim3(grid), dim3(256), 0, ctx->stream, m.rowptr.p, m.col.p, m.K.p, m.M.p, p, m.n,
                     k1 / mu, beta / mu, k2 / mu, r);
  PPH_HIP(ctx, hipGetLastError());
  return PPH_OK;
}

static int upload(pph_ctx* ctx, DevBuf<double>& d, const double* host, size_t count) {
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  PPH_TRY(d.alloc(ctx, count));
  PPH_HIP(ctx, hipMemcpyAsync(d.p, host, sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
  return PPH_OK;
}

extern "C" int pph_integrate_device(pph_ctx* ctx, const double* nodal_dev, double* out) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(flux_check(ctx, "pph_integrate_device", nodal_dev && out));
  DevBuf<double> part;
  const int st = integrate_dev(ctx, part, nodal_dev, out);
  part.release();
  return st;
}

extern "C" int pph_integrate(pph_ctx* ctx, const double* nodal_host, double* out) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(flux_check(ctx, "pph_integrate", nodal_host && out));
  DevBuf<double> u, part;
  int st = upload(ctx, u, nodal_host, (size_t)ctx->mesh.n);
  if (st == PPH_OK) st = integrate_dev(ctx, part, u.p, out);
  u.release(); part.release();
  return st;
}

extern "C" int pph_boundary_flux_device(pph_ctx* ctx, const double* nodal_dev, double conductivity, double* out) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(flux_check(ctx, "pph_boundary_flux_device", nodal_dev && out));
  DevBuf<double> part;
  const int st = boundary_flux_dev(ctx, part, nodal_dev, conductivity, out);
  part.release();
  return st;
}

extern "C" int pph_boundary_flux(pph_ctx* ctx, const double* nodal_host, double conductivity, double* out) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(flux_check(ctx, "pph_boundary_flux", nodal_host && out));
  DevBuf<double> u, part;
  int st = upload(ctx, u, nodal_host, (size_t)ctx->mesh.n);
  if (st == PPH_OK) st = boundary_flux_dev(ctx, part, u.p, conductivity, out);
  u.release(); part.release();
  return st;
}

extern "C" int pph_dpp_nodal_flux_device(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p_dev,
                                         double* r_dev) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(flux_check(ctx, "pph_dpp_nodal_flux_device", p_dev && r_dev));
  PPH_REQUIRE(ctx, mu != 0.0, "pph_dpp_nodal_flux_device: mu must not be 0");
  PPH_TRY(pph_nodal_flux_launch(ctx, k1, k2, beta, mu, p_dev, r_dev));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the caller's arrays are free again when the call returns)
  return PPH_OK;
}

extern "C" int pph_dpp_nodal_flux(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p_host,
                                  double* r_host) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(flux_check(ctx, "pph_dpp_nodal_flux", p_host && r_host));
  PPH_REQUIRE(ctx, mu != 0.0, "pph_dpp_nodal_flux: mu must not be 0");
  const size_t n2 = 2 * (size_t)ctx->mesh.n;
  DevBuf<double> p, r;
  int st = upload(ctx, p, p_host, n2);
  if (st == PPH_OK) st = r.alloc(ctx, n2);
  if (st == PPH_OK) st = pph_nodal_flux_launch(ctx, k1, k2, beta, mu, p.p, r.p);
  if (st == PPH_OK) {
    hipError_t e = hipMemcpyAsync(r_host, r.p, sizeof(double) * n2, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      pph_set_error(ctx, "pph_dpp_nodal_flux: copy of the result failed: %s", hipGetErrorString(e));
      st = PPH_ERR_HIP;
    }
  }
  p.release(); r.release();
  return st;
}
