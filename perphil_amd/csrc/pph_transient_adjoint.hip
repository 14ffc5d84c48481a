// Transient adjoint: gradients of functionals of a theta-stepped trajectory (pph_transient.hip) with respect to k1, k2, beta,
// mu, the storage coefficients, the initial field and the boundary data.
//
// No reference counterpart: the reference solves the steady state of dpp_form (src/perphil/forms/dpp.py:95-132).  Forward, as
// pph_transient_steps runs it: d_s = T^-1 (-F A_unel p_s), p_{s+1} = p_s + d_s, T = Sigma M / dt + theta A symmetric and
// assembled once.  For J = sum_s j_s(p_s), G_s = dj_s / dp_s, the discrete adjoint is one solve per step with the SAME operator
// and preconditioner, s = N-1 down to 0 from q_N = F G_N:
//   w_s = T^-1 q_{s+1}                                   (0 on constrained dofs; q = 0 gives w = 0 without a Krylov loop)
//   pm = p_s + theta d_s,  d_s = p_{s+1} - p_s
//   O0 = w1^T K pm1   O1 = w2^T K pm2   O2 = (w1 - w2)^T M (pm1 - pm2)   O3 = w1^T M d1   O4 = w2^T M d2      (terms[s])
//   q_s = F G_s + q_{s+1} - F A_unel w_s,   Wsum += w_s
//   dJ/dk1 = -sum O0 / mu, dJ/dk2 = -sum O1 / mu, dJ/dbeta = -sum O2 / mu, dJ/dmu = (k1 O0 + k2 O1 + beta O2) / mu^2,
//   dJ/dS1 = -sum O3 / dt, dJ/dS2 = -sum O4 / dt, dJ/dp_0 = q_0 on free dofs,
//   dJ/d(boundary value at constrained dof c) = sum_s (G_s)_c - (A_unel Wsum)_c.
//
//   k_transient_bilinear   the five forms of one step in one matrix-free pass over the boxes: w, p_s, p_{s+1} (2n each) and the
//                          dof map are read, pm and d are formed in registers while gathering, nothing of K or M is stored.  The
//                          element forms are pph_bilinear.h's (shared with k_dpp_bilinear).  HBM traffic per box: the dof map
//                          (4 B x nodes per box) and, amortised over the boxes that share a node, 6 doubles per node.
//                          Registers: every cell but the Q2 hexahedron holds its 6 gathered fields at once (at most 10 x 6 = 60
//                          doubles, P2 tetrahedra); 27 x 6 cannot be held: there the five forms run one after the other, each
//                          gathering where it uses a value, as the ONE_PASS == false branch of k_dpp_bilinear does.
//                          Determinism: k_dpp_bilinear's layout - grid-stride boxes, a fixed LDS tree, per-workgroup partial
//                          sums, k_bilinear_sum in a fixed order; the grid is a function of the mesh alone.  No atomics.
//   k_eval_points_adjoint  the transpose of pph_eval_points: out[node] += phi_a(x_m) c[m].  ONE workgroup takes the points in
//                          index order, lanes are the local basis functions (distinct nodes of one cell), a barrier separates
//                          points: no atomics, bitwise reproducible, any number of points per cell.  Cost LINEAR in m (serial over
//                          the points): it is meant for wells - tens to thousands of points.  Location, ties and tol are
//                          pph_eval_points' (pph_locate.h); a point outside contributes nothing and is counted.
//   the loop               pph_transient_adjoint*: exchange of the context's vectors once per call (as transient_run), per step
//                          one solve on the path cfg names, the bilinear kernel into a device array of terms (fetched once at
//                          the end), k_step_rhs on w and ONE pass for q_s and Wsum (k_adj_update).  Per step the host reads
//                          ||q||^2 once, beside the solve's own synchronisations.
#include "pph_internal.h"
#include "pph_locate.h"
#include "pph_p2.h"
#include "pph_bilinear.h"
#include <string>

#define ADJ_MAX_BLOCKS 2048   // grid cap of the vector passes

template <int KIND, int DEG>
struct TbCell {
  static constexpr bool ONE_PASS = (6 * BlCell<KIND, DEG>::NB <= 64);   // six gathered fields of a cell fit in registers
};

// part[q * BL_MAX_BLOCKS + block]: this workgroup's share of O_q, q < 5; w, p0 (= p_s), p1 (= p_{s+1}): 2n values, field-major
template <int KIND, int DEG>
__global__ __launch_bounds__(256, 1) void k_transient_bilinear(
    const int32_t* __restrict__ cells, const double* __restrict__ w, const double* __restrict__ p0, const double* __restrict__ p1,
    double theta, int64_t n, int64_t nbox, BlGeo g, BlTab tab, double* __restrict__ part) {
  using C = BlCell<KIND, DEG>;
  constexpr int NB = C::NB;
  __shared__ double lds[256];
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t box = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; box < nbox; box += (int64_t)gridDim.x * blockDim.x) {
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int sub = 0; sub < C::CPB; ++sub) {
      const int32_t* cn = cells + (box * C::CPB + sub) * NB;
      int32_t id[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) id[k] = cn[k];
      if constexpr (TbCell<KIND, DEG>::ONE_PASS) {
        double w1[NB], w2[NB], m1[NB], m2[NB], d1[NB], d2[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          const double a1 = p0[id[k]], a2 = p0[n + id[k]];
          d1[k] = p1[id[k]] - a1;
          d2[k] = p1[n + id[k]] - a2;
          m1[k] = a1 + theta * d1[k];
          m2[k] = a2 + theta * d2[k];
          w1[k] = w[id[k]];
          w2[k] = w[n + id[k]];
        }
        s[0] += bl_stiff<KIND, DEG>([&](int k) { return w1[k]; }, [&](int k) { return m1[k]; }, g, sub);
        s[1] += bl_stiff<KIND, DEG>([&](int k) { return w2[k]; }, [&](int k) { return m2[k]; }, g, sub);
        s[2] += bl_mass<KIND, DEG>([&](int k) { return w1[k] - w2[k]; }, [&](int k) { return m1[k] - m2[k]; }, g, tab);
        s[3] += bl_mass<KIND, DEG>([&](int k) { return w1[k]; }, [&](int k) { return d1[k]; }, g, tab);
        s[4] += bl_mass<KIND, DEG>([&](int k) { return w2[k]; }, [&](int k) { return d2[k]; }, g, tab);
      } else {
        // one form at a time, each value gathered where the form uses it (the scheduling barriers keep the next form's
        // gathers from being hoisted over this one's work; behind an opaque copy of the pointers the loads are issued again
        // instead of their first results being kept alive across forms)
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          s[f] += bl_stiff<KIND, DEG>([&](int k) { return w[f * n + id[k]]; },
                                      [&](int k) { const double a = p0[f * n + id[k]]; return a + theta * (p1[f * n + id[k]] - a); },
                                      g, sub);
          __builtin_amdgcn_sched_barrier(0);
        }
        {
          const double *w3 = w, *a3 = p0, *b3 = p1;
          asm volatile("" : "+s"(w3), "+s"(a3), "+s"(b3));
          s[2] += bl_mass<KIND, DEG>([&](int k) { return w3[id[k]] - w3[n + id[k]]; },
                                     [&](int k) {
                                       const double a1 = a3[id[k]], a2 = a3[n + id[k]];
                                       return (a1 + theta * (b3[id[k]] - a1)) - (a2 + theta * (b3[n + id[k]] - a2));
                                     }, g, tab);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const double *w4 = w, *a4 = p0, *b4 = p1;
          asm volatile("" : "+s"(w4), "+s"(a4), "+s"(b4));
          s[3 + f] += bl_mass<KIND, DEG>([&](int k) { return w4[f * n + id[k]]; },
                                         [&](int k) { return b4[f * n + id[k]] - a4[f * n + id[k]]; }, g, tab);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[q] += s[q];
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const double t = bl_block_sum(acc[q], lds);
    if (threadIdx.x == 0) part[(int64_t)q * BL_MAX_BLOCKS + blockIdx.x] = t;
  }
}

template <int KIND>
static void tb_launch(pph_ctx* ctx, int degree, int grid, const double* w, const double* p0, const double* p1, double theta,
                      int64_t nbox, const BlGeo& g, const BlTab& tab, double* part) {
  const int32_t* cells = ctx->mesh.cells.p;
  if (degree == 2)
    hipLaunchKernelGGL((k_transient_bilinear<KIND, 2>), dim3(grid), dim3(256), 0, ctx->stream, cells, w, p0, p1, theta, ctx->mesh.n,
                       nbox, g, tab, part);
  else
    hipLaunchKernelGGL((k_transient_bilinear<KIND, 1>), dim3(grid), dim3(256), 0, ctx->stream, cells, w, p0, p1, theta, ctx->mesh.n,
                       nbox, g, tab, part);
}

// enqueues the kernel and the second stage: res[0..4] (device) = the five forms; part: 5 * BL_MAX_BLOCKS doubles
static int tb_enqueue(pph_ctx* ctx, double* part, const double* w, const double* p0, const double* p1, double theta, double* res) {
  const MeshData& m = ctx->mesh;
  const int nd[3] = {m.nx, m.ny, (m.dim == 3) ? m.nzl : 1};
  const int64_t nbox = (int64_t)nd[0] * nd[1] * nd[2];
  const int cpb = p2_cells_per_box(m.kind);
  BlGeo g;
  g.vol = 1.0 / ((double)nbox * (double)cpb);
  for (int d = 0; d < 3; ++d) g.cd[d] = (d < m.dim) ? (double)nd[d] * (double)nd[d] * g.vol : 0.0;
  BlTab tab;
  bl_p2_mass_table(m.dim, &tab);
  const int64_t nb = ceil_div64(nbox, 256);
  const int grid = (int)(nb < 1 ? 1 : (nb < BL_MAX_BLOCKS ? nb : BL_MAX_BLOCKS));
  if (m.kind == PPH_CELL_QUAD) tb_launch<PPH_CELL_QUAD>(ctx, m.degree, grid, w, p0, p1, theta, nbox, g, tab, part);
  else if (m.kind == PPH_CELL_TRI) tb_launch<PPH_CELL_TRI>(ctx, m.degree, grid, w, p0, p1, theta, nbox, g, tab, part);
  else if (m.kind == PPH_CELL_HEX) tb_launch<PPH_CELL_HEX>(ctx, m.degree, grid, w, p0, p1, theta, nbox, g, tab, part);
  else tb_launch<PPH_CELL_TET>(ctx, m.degree, grid, w, p0, p1, theta, nbox, g, tab, part);
  hipLaunchKernelGGL(k_bilinear_sum, dim3(5), dim3(256), 0, ctx->stream, part, grid, res);
  PPH_HIP(ctx, hipGetLastError());
  return PPH_OK;
}

static int tb_check(pph_ctx* ctx, const char* who, bool buffers) {
  PPH_REQUIRE(ctx, ctx->mesh_ok, "%s before pph_mesh_build", who);
  PPH_REQUIRE(ctx, ctx->world == 1, "%s is implemented for single-context meshes", who);
  PPH_REQUIRE(ctx, buffers, "%s: NULL buffer", who);
  return PPH_OK;
}

static int tb_dev(pph_ctx* ctx, DevBuf<double>& part, const double* w, const double* p0, const double* p1, double theta,
                  double* out5) {
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  PPH_TRY(part.alloc(ctx, (size_t)5 * BL_MAX_BLOCKS + 5));
  double* res = part.p + (size_t)5 * BL_MAX_BLOCKS;
  PPH_TRY(tb_enqueue(ctx, part.p, w, p0, p1, theta, res));
  PPH_HIP(ctx, hipMemcpyAsync(out5, res, 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PPH_OK;
}

extern "C" int pph_transient_bilinear_device(pph_ctx* ctx, const double* w_dev, const double* p0_dev, const double* p1_dev,
                                             double theta, double* out5) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(tb_check(ctx, "pph_transient_bilinear_device", w_dev && p0_dev && p1_dev && out5));
  DevBuf<double> part;
  const int st = tb_dev(ctx, part, w_dev, p0_dev, p1_dev, theta, out5);
  part.release();
  return st;
}

extern "C" int pph_transient_bilinear(pph_ctx* ctx, const double* w_host, const double* p0_host, const double* p1_host,
                                      double theta, double* out5) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(tb_check(ctx, "pph_transient_bilinear", w_host && p0_host && p1_host && out5));
  const size_t n2 = 2 * (size_t)ctx->mesh.n;
  DevBuf<double> v, part;   // w, p0, p1
  int st = PPH_OK;
  auto upload = [&]() -> int {
    PPH_HIP(ctx, hipSetDevice(ctx->device));
    PPH_TRY(v.alloc(ctx, 3 * n2));
    PPH_HIP(ctx, hipMemcpyAsync(v.p, w_host, sizeof(double) * n2, hipMemcpyHostToDevice, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(v.p + n2, p0_host, sizeof(double) * n2, hipMemcpyHostToDevice, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(v.p + 2 * n2, p1_host, sizeof(double) * n2, hipMemcpyHostToDevice, ctx->stream));
    return PPH_OK;
  };
  st = upload();
  if (st == PPH_OK) st = tb_dev(ctx, part, v.p, v.p + n2, v.p + 2 * n2, theta, out5);
  else (void)hipStreamSynchronize(ctx->stream);   // (a copy may still read the caller's array)
  v.release(); part.release();
  return st;
}

// ---- transposed point evaluation -------------------------------------------------------------------------------------
// (the basis values of a located point: adj_basis, pph_locate.h - shared with pph_sources.hip)
// out[node * os_node + comp * os_comp] += N_a(x_p) c[p * ncomp + comp] for the nodes a of the cell that holds x_p; ONE workgroup
// of one wave, points in index order.  *n_outside = number of points outside (written, not added)
template <int KIND, int DEG>
__global__ __launch_bounds__(64) void k_eval_points_adjoint(const int32_t* __restrict__ cells, const double* __restrict__ x,
                                                            int64_t m, const double* __restrict__ c, int ncomp, int64_t os_node,
                                                            int64_t os_comp, EvalGeo g, double tol, double* out,
                                                            unsigned long long* __restrict__ n_outside) {
  using C = BlCell<KIND, DEG>;
  constexpr int DIM = C::DIM, NB = C::NB, CPB = C::CPB;
  const int lane = threadIdx.x;
  unsigned long long outside = 0;
  for (int64_t p = 0; p < m; ++p) {   // (every lane walks every point: the branches below are uniform)
    double xi[3] = {0.0, 0.0, 0.0};
    int64_t box = 0, stride = 1;
    bool outp = false;
#pragma unroll
    for (int e = 0; e < DIM; ++e) {
      double cb;
      const double s = box_locate(x[p * DIM + e], g.n[e], &cb);
      outp = outp || !(s >= -tol && s <= 1.0 + tol);
      xi[e] = fmin(fmax(s, 0.0), 1.0);
      box += stride * (int64_t)cb;
      stride *= g.n[e];
    }
    if (outp) { ++outside; continue; }
    double N[NB];
    const int sub = adj_basis<KIND, DEG, NB>(xi, N);
    double mine = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) mine = (b == lane) ? N[b] : mine;
    if (lane < NB) {
      const int64_t node = cells[(box * CPB + sub) * NB + lane];
      for (int q = 0; q < ncomp; ++q) out[node * os_node + q * os_comp] += mine * c[p * ncomp + q];
    }
    __syncthreads();   // (the next point may touch the same nodes from other lanes)
  }
  if (lane == 0) *n_outside = outside;
}

template <int KIND>
static void epa_launch(pph_ctx* ctx, int degree, const double* x, int64_t m, const double* c, int ncomp, int64_t os_node,
                       int64_t os_comp, EvalGeo g, double tol, double* out, unsigned long long* cnt) {
  const int32_t* cells = ctx->mesh.cells.p;
  if (degree == 2)
    hipLaunchKernelGGL((k_eval_points_adjoint<KIND, 2>), dim3(1), dim3(64), 0, ctx->stream, cells, x, m, c, ncomp, os_node, os_comp, g,
                       tol, out, cnt);
  else
    hipLaunchKernelGGL((k_eval_points_adjoint<KIND, 1>), dim3(1), dim3(64), 0, ctx->stream, cells, x, m, c, ncomp, os_node, os_comp, g,
                       tol, out, cnt);
}

// enqueued on the context stream; cnt: one device counter
static int epa_enqueue(pph_ctx* ctx, const double* x, int64_t m, const double* c, int ncomp, int64_t os_node, int64_t os_comp,
                       double tol, double* out, unsigned long long* cnt) {
  const MeshData& ms = ctx->mesh;
  EvalGeo g;
  g.n[0] = ms.nx; g.n[1] = ms.ny; g.n[2] = (ms.dim == 3) ? ms.nzl : 1;
  if (ms.kind == PPH_CELL_QUAD) epa_launch<PPH_CELL_QUAD>(ctx, ms.degree, x, m, c, ncomp, os_node, os_comp, g, tol, out, cnt);
  else if (ms.kind == PPH_CELL_TRI) epa_launch<PPH_CELL_TRI>(ctx, ms.degree, x, m, c, ncomp, os_node, os_comp, g, tol, out, cnt);
  else if (ms.kind == PPH_CELL_HEX) epa_launch<PPH_CELL_HEX>(ctx, ms.degree, x, m, c, ncomp, os_node, os_comp, g, tol, out, cnt);
  else epa_launch<PPH_CELL_TET>(ctx, ms.degree, x, m, c, ncomp, os_node, os_comp, g, tol, out, cnt);
  PPH_HIP(ctx, hipGetLastError());
  return PPH_OK;
}

static int epa_check(pph_ctx* ctx, const char* who, const void* x, int64_t m, const void* c, int ncomp, double tol, const void* out,
                     const int64_t* n_outside) {
  PPH_REQUIRE(ctx, ctx->mesh_ok, "%s before pph_mesh_build", who);
  PPH_REQUIRE(ctx, ctx->world == 1, "point evaluation is implemented for single-context meshes");
  PPH_REQUIRE(ctx, out && n_outside && m >= 0 && (m == 0 || (x && c)), "%s: NULL buffer or negative point count", who);
  PPH_REQUIRE(ctx, ncomp >= 1, "%s: ncomp must be at least 1, got %d", who, ncomp);
  PPH_REQUIRE(ctx, tol >= 0.0 && tol < 0.5, "%s: tol must be in [0, 0.5) box-local units", who);
  return PPH_OK;
}

struct EpaBufs {
  DevBuf<double> v;   // host variant: out, x, c
  DevBuf<unsigned long long> cnt;
  unsigned long long h = 0;
  void release() { v.release(); cnt.release(); }
};

static int epa_device(pph_ctx* ctx, EpaBufs& b, const double* x, int64_t m, const double* c, int ncomp, double tol, double* out,
                      int64_t* n_outside) {
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  *n_outside = 0;
  if (m == 0) return PPH_OK;
  PPH_TRY(b.cnt.alloc(ctx, 1));
  PPH_TRY(epa_enqueue(ctx, x, m, c, ncomp, ncomp, 1, tol, out, b.cnt.p));
  PPH_HIP(ctx, hipMemcpyAsync(&b.h, b.cnt.p, sizeof(b.h), hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *n_outside = (int64_t)b.h;
  return PPH_OK;
}

static int epa_host(pph_ctx* ctx, EpaBufs& b, const double* x_host, int64_t m, const double* c_host, int ncomp, double tol,
                    double* out_host, int64_t* n_outside) {
  const MeshData& ms = ctx->mesh;
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  *n_outside = 0;
  if (m == 0) return PPH_OK;
  const size_t no = (size_t)ms.n * ncomp, nx = (size_t)m * ms.dim, nc = (size_t)m * ncomp;
  PPH_TRY(b.v.alloc(ctx, no + nx + nc));
  PPH_TRY(b.cnt.alloc(ctx, 1));
  double *out = b.v.p, *x = out + no, *c = x + nx;
  PPH_HIP(ctx, hipMemcpyAsync(out, out_host, sizeof(double) * no, hipMemcpyHostToDevice, ctx->stream));
  PPH_HIP(ctx, hipMemcpyAsync(x, x_host, sizeof(double) * nx, hipMemcpyHostToDevice, ctx->stream));
  PPH_HIP(ctx, hipMemcpyAsync(c, c_host, sizeof(double) * nc, hipMemcpyHostToDevice, ctx->stream));
  PPH_TRY(epa_enqueue(ctx, x, m, c, ncomp, ncomp, 1, tol, out, b.cnt.p));
  PPH_HIP(ctx, hipMemcpyAsync(out_host, out, sizeof(double) * no, hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipMemcpyAsync(&b.h, b.cnt.p, sizeof(b.h), hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *n_outside = (int64_t)b.h;
  return PPH_OK;
}

extern "C" int pph_eval_points_adjoint_device(pph_ctx* ctx, const double* x_dev, int64_t m, const double* c_dev, int ncomp,
                                              double tol, double* out_dev, int64_t* n_outside) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(epa_check(ctx, "pph_eval_points_adjoint_device", x_dev, m, c_dev, ncomp, tol, out_dev, n_outside));
  EpaBufs b;
  int st = epa_device(ctx, b, x_dev, m, c_dev, ncomp, tol, out_dev, n_outside);
  if (st < 0) (void)hipStreamSynchronize(ctx->stream);
  b.release();
  return st;
}

extern "C" int pph_eval_points_adjoint(pph_ctx* ctx, const double* x_host, int64_t m, const double* c_host, int ncomp, double tol,
                                       double* out_host, int64_t* n_outside) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(epa_check(ctx, "pph_eval_points_adjoint", x_host, m, c_host, ncomp, tol, out_host, n_outside));
  EpaBufs b;
  int st = epa_host(ctx, b, x_host, m, c_host, ncomp, tol, out_host, n_outside);
  if (st < 0) (void)hipStreamSynchronize(ctx->stream);   // (a copy may still read the caller's array)
  b.release();
  return st;
}

// ---- the backward loop -------------------------------------------------------------------------------------------------
// dst = (mask != 0) ? 0 : src over both fields
__global__ __launch_bounds__(256) void k_adj_mask(double* __restrict__ dst, const double* __restrict__ src,
                                                  const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 2 * n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t m = (i < n) ? m0[i] : m1[i - n];
    dst[i] = m ? 0.0 : src[i];
  }
}

// q = F (G + q + b) and wsum += w in one pass; G, b, w / wsum may be NULL (taken as 0 / skipped).  b = -F A_unel w is what
// k_step_rhs wrote for the input w
__global__ __launch_bounds__(256) void k_adj_update(double* __restrict__ q, const double* __restrict__ G, const double* __restrict__ b,
                                                    const double* __restrict__ w, double* __restrict__ wsum,
                                                    const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 2 * n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t m = (i < n) ? m0[i] : m1[i - n];
    const double gi = G ? G[i] : 0.0, bi = b ? b[i] : 0.0;
    q[i] = m ? 0.0 : (gi + q[i]) + bi;
    if (wsum) wsum[i] += w[i];
  }
}

struct AdjArgs {
  const double *traj, *g, *obs_x, *obs_c;
  int64_t m;
  double tol;
  int nsteps;
  double *q0, *wsum;
  pph_solve_info* infos;
  int* steps_done;
  // rate gradients (pph_sources.hip): NULL, or src_grad [nsteps][K] on the device and the scratch of its partial sums
  double *src_grad = nullptr, *src_part = nullptr;
  int64_t K = 0;
};

// the loop between the exchange and the restore.  work: save (3 x 2n) | q | w | b | G | part (5 x BL_MAX_BLOCKS) | terms (5 N)
// (| the partial sums of the rate gradients | src_grad (N K))
static int adjoint_run(pph_ctx* ctx, const pph_solver_cfg* cfg, const AdjArgs& a, double* work, unsigned long long* cnt) {
  const int64_t n = ctx->n, N = 2 * n;
  const int grid = (int)(ceil_div64(N, 256) < ADJ_MAX_BLOCKS ? ceil_div64(N, 256) : ADJ_MAX_BLOCKS);
  double *save = work, *q = work + 3 * N, *w = q + N, *b = w + N, *G = b + N, *part = G + N;
  double* terms = part + (size_t)5 * BL_MAX_BLOCKS;
  const uint8_t *m0 = ctx->bcmask[0].p, *m1 = ctx->bcmask[1].p;
  la_copy(ctx, save, ctx->rhs.p, N);
  la_copy(ctx, save + N, ctx->u0.p, N);
  la_copy(ctx, save + 2 * N, ctx->sol.p, N);
  la_set(ctx, ctx->u0.p, 0.0, N);
  la_set(ctx, q, 0.0, N);
  if (a.wsum) la_set(ctx, a.wsum, 0.0, N);
  PPH_HIP(ctx, hipGetLastError());
  // G_s = g[s] + E^T obs_c[s]: the caller's row where there are no observations, else formed in G
  auto functional = [&](int s, const double** Gs) -> int {
    *Gs = a.g ? a.g + (int64_t)s * N : nullptr;
    if (!a.obs_c || a.m == 0) return PPH_OK;
    if (a.g) la_copy(ctx, G, a.g + (int64_t)s * N, N);
    else la_set(ctx, G, 0.0, N);
    PPH_TRY(epa_enqueue(ctx, a.obs_x, a.m, a.obs_c + (int64_t)s * a.m * 2, 2, 1, n, a.tol, G, cnt));
    *Gs = G;
    return PPH_OK;
  };
  const double* Gs = nullptr;
  PPH_TRY(functional(a.nsteps, &Gs));
  hipLaunchKernelGGL(k_adj_update, dim3(grid), dim3(256), 0, ctx->stream, q, Gs, (const double*)nullptr, (const double*)nullptr,
                     (double*)nullptr, m0, m1, n);
  PPH_HIP(ctx, hipGetLastError());
  int st = PPH_OK, done = 0;
  for (int s = a.nsteps - 1; s >= 0; --s) {
    la_copy(ctx, ctx->rhs.p, q, N);
    la_dot(ctx, ctx->rhs.p, ctx->rhs.p, N, 0);
    PPH_TRY(la_fetch(ctx, 0, 1));
    pph_solve_info info;
    info.iterations = 0; info.inner_iterations = 0; info.converged = 1; info.inner_failed = 0; info.resnorm = 0.0; info.rhs_norm = 0.0;
    if (ctx->h_scal[0] != 0.0) {   // (q without an entry on a free dof: w = 0 without entering a Krylov loop)
      st = pph_solve_device(ctx, cfg, &info, nullptr, 0);
      if (st < 0 && st != PPH_ERR_DIVERGED) return st;
      hipLaunchKernelGGL(k_adj_mask, dim3(grid), dim3(256), 0, ctx->stream, w, ctx->sol.p, m0, m1, n);
    } else {
      la_set(ctx, w, 0.0, N);
    }
    if (a.infos) a.infos[s] = info;
    if (st == PPH_ERR_DIVERGED) break;
    PPH_TRY(tb_enqueue(ctx, part, w, a.traj + (int64_t)s * N, a.traj + (int64_t)(s + 1) * N, ctx->tr_theta, terms + 5 * s));
    if (a.src_grad) PPH_TRY(src_dot_launch(ctx, w, a.src_part, a.src_grad + (int64_t)s * a.K));   // src_grad[s][k] = w_s^T F L_k
    PPH_TRY(pph_step_rhs_launch(ctx, ctx->tr_coef[0], ctx->tr_coef[1], ctx->tr_coef[2], ctx->tr_coef[3], w, b));
    PPH_TRY(functional(s, &Gs));
    hipLaunchKernelGGL(k_adj_update, dim3(grid), dim3(256), 0, ctx->stream, q, Gs, (const double*)b, (const double*)w, a.wsum, m0, m1, n);
    PPH_HIP(ctx, hipGetLastError());
    ++done;
  }
  *a.steps_done = done;
  la_copy(ctx, a.q0, q, N);
  PPH_HIP(ctx, hipGetLastError());
  return st;
}

static int adjoint_check(pph_ctx* ctx, const pph_solver_cfg* cfg, const void* traj, const void* g, const void* obs_x, int64_t m,
                         const void* obs_c, double tol, int nsteps, const void* terms, const void* q0, const int* steps_done) {
  PPH_REQUIRE(ctx, ctx->world == 1, "pph_transient_adjoint is implemented for single-context meshes");
  PPH_REQUIRE(ctx, ctx->tr_on, "pph_transient_adjoint before pph_transient_begin");
  PPH_REQUIRE(ctx, ctx->asm_ok && ctx->asm_epoch == ctx->tr_asm_epoch,
              "pph_transient_adjoint: the system was assembled again (or dropped) after pph_transient_begin");
  PPH_REQUIRE(ctx, ctx->bc_epoch == ctx->tr_bc_epoch, "pph_transient_adjoint: the Dirichlet sets changed after pph_transient_begin");
  PPH_REQUIRE(ctx, traj && terms && q0 && steps_done && cfg, "pph_transient_adjoint: NULL buffer");
  PPH_REQUIRE(ctx, g || obs_c, "pph_transient_adjoint: neither g nor the observation form is given");
  PPH_REQUIRE(ctx, !obs_c || (m >= 0 && (m == 0 || obs_x)), "pph_transient_adjoint: obs_c without obs_x, or a negative point count");
  PPH_REQUIRE(ctx, tol >= 0.0 && tol < 0.5, "pph_transient_adjoint: obs_tol must be in [0, 0.5) box-local units");
  PPH_REQUIRE(ctx, nsteps >= 1, "pph_transient_adjoint: nsteps must be >= 1, got %d", nsteps);
  return validate_cfg(ctx, cfg);
}

// the checks of the variants with rate gradients (pph_transient_adjoint_sources*), after adjoint_check
static int adjoint_sources_check(pph_ctx* ctx, const double* src_grad, int64_t K) {
  PPH_REQUIRE(ctx, ctx->src.on, "pph_transient_adjoint_sources: the context holds no source set (pph_sources_set)");
  PPH_REQUIRE(ctx, ctx->src.count() == K, "pph_transient_adjoint_sources: src_grad has %lld columns, the context's source set %lld sources",
              (long long)K, (long long)ctx->src.count());
  PPH_REQUIRE(ctx, K == 0 || src_grad != nullptr, "pph_transient_adjoint_sources: NULL buffer");
  return PPH_OK;
}

// `sources`: also src_grad [nsteps][K] (host), written on the device per step and fetched once, as terms
static int adjoint_device(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* traj_dev, const double* g_dev,
                          const double* obs_x_dev, int64_t m, const double* obs_c_dev, double obs_tol, int nsteps, double* terms,
                          double* q0_dev, double* wsum_dev, pph_solve_info* infos, int* steps_done, bool sources, double* src_grad,
                          int64_t K) {
  if (steps_done) *steps_done = 0;
  PPH_TRY(adjoint_check(ctx, cfg, traj_dev, g_dev, obs_x_dev, m, obs_c_dev, obs_tol, nsteps, terms, q0_dev, steps_done));
  if (sources) PPH_TRY(adjoint_sources_check(ctx, src_grad, K));
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t N = 2 * ctx->n;
  const bool sg = sources && K > 0;
  const size_t n_base = (size_t)(7 * N) + (size_t)5 * BL_MAX_BLOCKS + (size_t)5 * nsteps;
  const size_t n_part = sg ? src_dot_part_count(ctx) : 0, n_sg = sg ? (size_t)nsteps * (size_t)K : 0;
  DevBuf<double> work;
  DevBuf<unsigned long long> cnt;
  PPH_TRY(work.alloc(ctx, n_base + n_part + n_sg));
  int st = cnt.alloc(ctx, 1);
  if (st < 0) { work.release(); return st; }
  AdjArgs a = {traj_dev, g_dev, obs_x_dev, obs_c_dev, m, obs_tol, nsteps, q0_dev, wsum_dev, infos, steps_done};
  if (sg) { a.src_part = work.p + n_base; a.src_grad = a.src_part + n_part; a.K = K; }
  st = adjoint_run(ctx, cfg, a, work.p, cnt.p);
  const std::string msg = ctx->err;   // (the solve's message survives the clean-up)
  // the context's right-hand side, lifting and solution again hold the bits they held before the call
  la_copy(ctx, ctx->rhs.p, work.p, N);
  la_copy(ctx, ctx->u0.p, work.p + N, N);
  la_copy(ctx, ctx->sol.p, work.p + 2 * N, N);
  hipError_t e = hipGetLastError();
  // the terms of the completed steps (s = nsteps - 1 down to nsteps - done), fetched once
  const int done = *steps_done;
  for (int i = 0; i < 5 * nsteps; ++i) terms[i] = 0.0;
  if (e == hipSuccess && done > 0 && (st >= 0 || st == PPH_ERR_DIVERGED)) {
    const double* tdev = work.p + 7 * N + (size_t)5 * BL_MAX_BLOCKS + (size_t)5 * (nsteps - done);
    e = hipMemcpyAsync(terms + (size_t)5 * (nsteps - done), tdev, sizeof(double) * 5 * done, hipMemcpyDeviceToHost, ctx->stream);
  }
  if (sg) {   // ... and the rate gradients of the same steps
    for (size_t i = 0; i < n_sg; ++i) src_grad[i] = 0.0;
    if (e == hipSuccess && done > 0 && (st >= 0 || st == PPH_ERR_DIVERGED))
      e = hipMemcpyAsync(src_grad + (size_t)K * (nsteps - done), a.src_grad + (size_t)K * (nsteps - done),
                         sizeof(double) * (size_t)K * done, hipMemcpyDeviceToHost, ctx->stream);
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);   // (work is freed below; the caller's arrays are free again)
  if (e == hipSuccess) e = es;
  work.release(); cnt.release();
  if (e != hipSuccess && st >= 0) {
    pph_set_error(ctx, "pph_transient_adjoint: restoring the context's vectors failed: %s", hipGetErrorString(e));
    return PPH_ERR_HIP;
  }
  if (st < 0) ctx->err = msg;
  return st;
}

extern "C" int pph_transient_adjoint_device(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* traj_dev, const double* g_dev,
                                            const double* obs_x_dev, int64_t m, const double* obs_c_dev, double obs_tol, int nsteps,
                                            double* terms, double* q0_dev, double* wsum_dev, pph_solve_info* infos,
                                            int* steps_done) {
  if (!ctx) return PPH_ERR_INVALID;
  return adjoint_device(ctx, cfg, traj_dev, g_dev, obs_x_dev, m, obs_c_dev, obs_tol, nsteps, terms, q0_dev, wsum_dev, infos, steps_done,
                        false, nullptr, 0);
}

extern "C" int pph_transient_adjoint_sources_device(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* traj_dev,
                                                    const double* g_dev, const double* obs_x_dev, int64_t m, const double* obs_c_dev,
                                                    double obs_tol, int nsteps, double* terms, double* q0_dev, double* wsum_dev,
                                                    pph_solve_info* infos, int* steps_done, double* src_grad, int64_t K) {
  if (!ctx) return PPH_ERR_INVALID;
  return adjoint_device(ctx, cfg, traj_dev, g_dev, obs_x_dev, m, obs_c_dev, obs_tol, nsteps, terms, q0_dev, wsum_dev, infos, steps_done,
                        true, src_grad, K);
}

static int adjoint_host(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* traj_host, const double* g_host,
                        const double* obs_x_host, int64_t m, const double* obs_c_host, double obs_tol, int nsteps, double* terms,
                        double* q0_host, double* wsum_host, pph_solve_info* infos, int* steps_done, bool sources, double* src_grad,
                        int64_t K) {
  if (steps_done) *steps_done = 0;
  PPH_TRY(adjoint_check(ctx, cfg, traj_host, g_host, obs_x_host, m, obs_c_host, obs_tol, nsteps, terms, q0_host, steps_done));
  if (sources) PPH_TRY(adjoint_sources_check(ctx, src_grad, K));
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = 2 * (size_t)ctx->n, rows = (size_t)nsteps + 1, dim = (size_t)ctx->mesh.dim;
  const bool obs = obs_c_host != nullptr && m > 0;
  const size_t n_traj = rows * N, n_g = g_host ? rows * N : 0, n_x = obs ? (size_t)m * dim : 0, n_c = obs ? rows * (size_t)m * 2 : 0;
  DevBuf<double> v;   // traj | g | obs_x | obs_c | q0 | wsum
  PPH_TRY(v.alloc(ctx, n_traj + n_g + n_x + n_c + 2 * N));
  double *traj = v.p, *g = traj + n_traj, *x = g + n_g, *c = x + n_x, *q0 = c + n_c, *wsum = q0 + N;
  hipError_t e = hipMemcpyAsync(traj, traj_host, sizeof(double) * n_traj, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && n_g) e = hipMemcpyAsync(g, g_host, sizeof(double) * n_g, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && obs) e = hipMemcpyAsync(x, obs_x_host, sizeof(double) * n_x, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && obs) e = hipMemcpyAsync(c, obs_c_host, sizeof(double) * n_c, hipMemcpyHostToDevice, ctx->stream);
  int st = PPH_OK;
  if (e == hipSuccess) {
    // (an observation form without points is an empty sum: it still counts as given)
    st = adjoint_device(ctx, cfg, traj, g_host ? g : nullptr, obs ? x : nullptr, obs ? m : 0, obs_c_host ? (obs ? c : traj) : nullptr,
                        obs_tol, nsteps, terms, q0, wsum_host ? wsum : nullptr, infos, steps_done, sources, src_grad, K);
    if (st >= 0 || st == PPH_ERR_DIVERGED) {
      e = hipMemcpyAsync(q0_host, q0, sizeof(double) * N, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess && wsum_host) e = hipMemcpyAsync(wsum_host, wsum, sizeof(double) * N, hipMemcpyDeviceToHost, ctx->stream);
    }
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  v.release();
  if (e != hipSuccess && st >= 0) {
    pph_set_error(ctx, "pph_transient_adjoint: copy failed: %s", hipGetErrorString(e));
    return PPH_ERR_HIP;
  }
  return st;
}

extern "C" int pph_transient_adjoint(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* traj_host, const double* g_host,
                                     const double* obs_x_host, int64_t m, const double* obs_c_host, double obs_tol, int nsteps,
                                     double* terms, double* q0_host, double* wsum_host, pph_solve_info* infos, int* steps_done) {
  if (!ctx) return PPH_ERR_INVALID;
  return adjoint_host(ctx, cfg, traj_host, g_host, obs_x_host, m, obs_c_host, obs_tol, nsteps, terms, q0_host, wsum_host, infos,
                      steps_done, false, nullptr, 0);
}

extern "C" int pph_transient_adjoint_sources(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* traj_host, const double* g_host,
                                             const double* obs_x_host, int64_t m, const double* obs_c_host, double obs_tol, int nsteps,
                                             double* terms, double* q0_host, double* wsum_host, pph_solve_info* infos,
                                             int* steps_done, double* src_grad, int64_t K) {
  if (!ctx) return PPH_ERR_INVALID;
  return adjoint_host(ctx, cfg, traj_host, g_host, obs_x_host, m, obs_c_host, obs_tol, nsteps, terms, q0_host, wsum_host, infos,
                      steps_done, true, src_grad, K);
}
