// Sources of the transient DPP runs: wells (point loads) and distributed sources (dense load vectors).
//
// No reference counterpart: the reference's dpp_form (src/perphil/forms/dpp.py:95-132) has no right-hand side beyond the
// Dirichlet lifting.  With rates r_k(t) (q > 0 injects) and load vectors L_k (2n, field-major, constant in time) a theta step
// in delta form solves
//   (Sigma M / dt + theta A) d = F (-A_unel p^s + sum_k c[s][k] L_k),   c[s][k] = theta r_k(t_{s+1}) + (1 - theta) r_k(t_s),
// F the projection that zeroes the constrained dofs: a load on a Dirichlet node pumps into the boundary condition and is
// dropped.  The operator, the preconditioners and the Krylov loops never see a source; the step loop (pph_transient.hip) adds
// the term to b_s between k_step_rhs and the norm of b_s, the backward loop (pph_transient_adjoint.hip) takes w_s^T F L_k.
//
//   point load   L[dof] = phi_dof(x_w) on the nodes of the cell that holds x_w, in network f: the transpose of pph_eval_points,
//                same location rule, tie-breaks and tol (pph_locate.h).  k_src_point_rows, one work item per point, writes the
//                point's nb dofs and basis values by the calls k_eval_points_adjoint makes, in its order (box_locate,
//                adj_basis); an outside point gets the dof -1 in every entry (an empty row) and is counted on the host.
//   by-dof CSR   the m x nb entries are fetched once and regrouped on the host by dof (a stable sort of the entries, which are
//                generated in point order: dof first, then point index), then uploaded.  ONE work item owns a touched dof and
//                walks its entries in that order: any number of wells per cell or per node, no floating-point atomics, the
//                same bits whatever the grid.  Set-up cost: one small kernel, 16 bytes per entry down (an int64 dof and a basis
//                value), 12 bytes per entry up (an int32 point and a basis value) plus 16 bytes per touched dof (row pointer
//                and dof), and a sort of the m nb entries.
//   dense load   any 2n vector, copied into the context ([n_dense][2n]).
//   k_src_dense  b += F sum_k c[k] L_k in one grid-stride pass over PAIRS of entries (2n is even): every L_k is read once, b is
//                read and written once, both as 16-byte accesses (b: where its address is a multiple of 16 - the step loop's
//                always is; a caller's array that is not takes 8-byte accesses, same arithmetic, same bits); the masks are read as k_step_update reads them; the sum over
//                k runs in index order in registers; the coefficients come from a device array (uniform per wave: K may be in
//                the thousands).  HBM traffic per step: 8 (n_dense + 2) bytes per entry, 1 byte of mask.
//   k_src_points b[dof] += sum_entries w c[point] unless the dof is constrained: a few microseconds for tens to thousands of wells.
//   rate gradients  G[k] = w^T F L_k.  Dense: k_src_dot (grid y = load k; per-workgroup partial sums through a fixed LDS tree)
//                and k_src_dot_sum (one workgroup per load, fixed order): the layout of k_step_update + k_step_sum.  Points:
//                k_src_point_dot, one work item per point over the by-point rows kept from the set-up.
// Determinism: every sum has one owner and a fixed order; two calls give the same bits, host and device variants agree.
#include "pph_internal.h"
#include "pph_locate.h"
#include "pph_bilinear.h"
#include <algorithm>
#include <numeric>
#include <vector>

#define SRC_MAX_BLOCKS 2048   // grid cap of the passes (256 work items per workgroup and pass; k_src_dense: 256 PAIRS of entries)
#define SRC_MAX_DENSE 65535   // dense loads of a set (k_src_dot takes the load from the grid's y index)

template <int KIND, int DEG>
__global__ __launch_bounds__(256) void k_src_point_rows(const int32_t* __restrict__ cells, const double* __restrict__ x,
                                                        const int32_t* __restrict__ field, int64_t m, int64_t n, EvalGeo g,
                                                        double tol, int64_t* __restrict__ dof, double* __restrict__ val) {
  using C = BlCell<KIND, DEG>;
  constexpr int DIM = C::DIM, NB = C::NB, CPB = C::CPB;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
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
    if (outp) {
#pragma unroll
      for (int b = 0; b < NB; ++b) { dof[p * NB + b] = -1; val[p * NB + b] = 0.0; }
      continue;
    }
    double N[NB];
    const int sub = adj_basis<KIND, DEG, NB>(xi, N);
    const int64_t off = field[p] ? n : 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      dof[p * NB + b] = off + cells[(box * CPB + sub) * NB + b];
      val[p * NB + b] = N[b];
    }
  }
}

// b += F sum_k c[k] L_k; pair j holds the entries 2j and 2j + 1 of the 2n.  WIDE: b is 16-byte aligned (the loads always are)
template <bool WIDE>
__global__ __launch_bounds__(256) void k_src_dense(const double* __restrict__ L, const double* __restrict__ c, int64_t nd,
                                                   const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int64_t n,
                                                   double* __restrict__ b) {
  const int64_t N = 2 * n;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = 2 * j, i1 = i0 + 1;
    const uint8_t ma = (i0 < n) ? m0[i0] : m1[i0 - n], mb = (i1 < n) ? m0[i1] : m1[i1 - n];
    double s0 = 0.0, s1 = 0.0;
    for (int64_t k = 0; k < nd; ++k) {
      double l0, l1;
      sell_ld2(L + k * N + i0, l0, l1);
      const double ck = c[k];
      s0 += ck * l0;
      s1 += ck * l1;
    }
    if constexpr (WIDE) {
      double b0, b1;
      sell_ld2(b + i0, b0, b1);
      sell_st2(b + i0, ma ? b0 : b0 + s0, mb ? b1 : b1 + s1);
    } else {
      const double b0 = b[i0], b1 = b[i1];
      b[i0] = ma ? b0 : b0 + s0;
      b[i1] = mb ? b1 : b1 + s1;
    }
  }
}

// one work item per touched dof: its entries in (point) order; c: the coefficients of the points
__global__ __launch_bounds__(256) void k_src_points(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ row_dof,
                                                    const int32_t* __restrict__ ent_pt, const double* __restrict__ ent_w,
                                                    const double* __restrict__ c, int64_t nrows, const uint8_t* __restrict__ m0,
                                                    const uint8_t* __restrict__ m1, int64_t n, double* __restrict__ b) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t dof = row_dof[r];
    double s = 0.0;
    for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) s += ent_w[e] * c[ent_pt[e]];
    const uint8_t mk = (dof < n) ? m0[dof] : m1[dof - n];
    if (!mk) b[dof] += s;
  }
}

// part[k * SRC_MAX_BLOCKS + block] = this workgroup's share of w^T F L_k, k = blockIdx.y
__global__ __launch_bounds__(256) void k_src_dot(const double* __restrict__ L, const double* __restrict__ w,
                                                 const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int64_t n,
                                                 double* __restrict__ part) {
  __shared__ double lds[256];
  const int64_t N = 2 * n;
  const double* Lk = L + (int64_t)blockIdx.y * N;
  double acc = 0.0;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = 2 * j, i1 = i0 + 1;
    const uint8_t ma = (i0 < n) ? m0[i0] : m1[i0 - n], mb = (i1 < n) ? m0[i1] : m1[i1 - n];
    double l0, l1, w0, w1;
    sell_ld2(Lk + i0, l0, l1);
    sell_ld2(w + i0, w0, w1);
    acc += ma ? 0.0 : w0 * l0;
    acc += mb ? 0.0 : w1 * l1;
  }
  lds[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * SRC_MAX_BLOCKS + blockIdx.x] = lds[0];
}

// out[k] = sum of part[k * SRC_MAX_BLOCKS + i], i < nblocks; one workgroup per load k, fixed order
__global__ __launch_bounds__(256) void k_src_dot_sum(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  __shared__ double lds[256];
  const double* p = part + (int64_t)blockIdx.x * SRC_MAX_BLOCKS;
  double v = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) v += p[i];
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = lds[0];
}

// out[p] = sum over the point's nb entries of val * w[dof], constrained dofs (and the entries of an outside point) skipped
__global__ __launch_bounds__(256) void k_src_point_dot(const int64_t* __restrict__ dof, const double* __restrict__ val, int nb,
                                                       int64_t m, const double* __restrict__ w, const uint8_t* __restrict__ m0,
                                                       const uint8_t* __restrict__ m1, int64_t n, double* __restrict__ out) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) {
      const int64_t d = dof[p * nb + b];
      if (d < 0) continue;
      const uint8_t mk = (d < n) ? m0[d] : m1[d - n];
      if (!mk) s += val[p * nb + b] * w[d];
    }
    out[p] = s;
  }
}

static int src_grid(int64_t items) {
  const int64_t nb = ceil_div64(items, 256);
  return (int)(nb < 1 ? 1 : (nb < SRC_MAX_BLOCKS ? nb : SRC_MAX_BLOCKS));
}

int src_apply_launch(pph_ctx* ctx, const double* coef_dev, double* b) {
  const SourceSet& S = ctx->src;
  const int64_t n = ctx->n;
  const uint8_t *m0 = ctx->bcmask[0].p, *m1 = ctx->bcmask[1].p;
  if (S.n_dense > 0) {
    if (((uintptr_t)b & 15) == 0)
      hipLaunchKernelGGL(k_src_dense<true>, dim3(src_grid(n)), dim3(256), 0, ctx->stream, (const double*)S.dense.p, coef_dev,
                         S.n_dense, m0, m1, n, b);
    else
      hipLaunchKernelGGL(k_src_dense<false>, dim3(src_grid(n)), dim3(256), 0, ctx->stream, (const double*)S.dense.p, coef_dev,
                         S.n_dense, m0, m1, n, b);
  }
  if (S.n_touched > 0)
    hipLaunchKernelGGL(k_src_points, dim3(src_grid(S.n_touched)), dim3(256), 0, ctx->stream, (const int64_t*)S.rowptr.p,
                       (const int64_t*)S.row_dof.p, (const int32_t*)S.ent_pt.p, (const double*)S.ent_w.p, coef_dev + S.n_dense,
                       S.n_touched, m0, m1, n, b);
  PPH_HIP(ctx, hipGetLastError());
  return PPH_OK;
}

size_t src_dot_part_count(const pph_ctx* ctx) { return (size_t)ctx->src.n_dense * SRC_MAX_BLOCKS; }

int src_dot_launch(pph_ctx* ctx, const double* w, double* part, double* out_dev) {
  const SourceSet& S = ctx->src;
  const int64_t n = ctx->n;
  const uint8_t *m0 = ctx->bcmask[0].p, *m1 = ctx->bcmask[1].p;
  if (S.n_dense > 0) {
    const int grid = src_grid(n);
    hipLaunchKernelGGL(k_src_dot, dim3(grid, (unsigned)S.n_dense), dim3(256), 0, ctx->stream, (const double*)S.dense.p, w, m0, m1, n,
                       part);
    hipLaunchKernelGGL(k_src_dot_sum, dim3((unsigned)S.n_dense), dim3(256), 0, ctx->stream, (const double*)part, grid, out_dev);
  }
  if (S.m > 0)
    hipLaunchKernelGGL(k_src_point_dot, dim3(src_grid(S.m)), dim3(256), 0, ctx->stream, (const int64_t*)S.pt_dof.p,
                       (const double*)S.pt_w.p, S.nb, S.m, w, m0, m1, n, out_dev + S.n_dense);
  PPH_HIP(ctx, hipGetLastError());
  return PPH_OK;
}

template <int KIND>
static void src_rows_launch(pph_ctx* ctx, const double* x, const int32_t* field, int64_t m, EvalGeo g, double tol, int64_t* dof,
                            double* val) {
  const int32_t* cells = ctx->mesh.cells.p;
  const int grid = src_grid(m);
  if (ctx->mesh.degree == 2)
    hipLaunchKernelGGL((k_src_point_rows<KIND, 2>), dim3(grid), dim3(256), 0, ctx->stream, cells, x, field, m, ctx->n, g, tol, dof, val);
  else
    hipLaunchKernelGGL((k_src_point_rows<KIND, 1>), dim3(grid), dim3(256), 0, ctx->stream, cells, x, field, m, ctx->n, g, tol, dof, val);
}

static int src_nb(const MeshData& ms) {
  if (ms.degree == 2) return ms.kind == PPH_CELL_QUAD ? 9 : ms.kind == PPH_CELL_TRI ? 6 : ms.kind == PPH_CELL_HEX ? 27 : 10;
  return ms.kind == PPH_CELL_QUAD ? 4 : ms.kind == PPH_CELL_TRI ? 3 : ms.kind == PPH_CELL_HEX ? 8 : 4;
}

static int src_set_check(pph_ctx* ctx, const char* who, const void* dense, int64_t n_dense, const void* x, const int32_t* field,
                         int64_t m, double tol, const int64_t* n_outside) {
  PPH_REQUIRE(ctx, ctx->mesh_ok, "%s before pph_mesh_build", who);
  PPH_REQUIRE(ctx, ctx->world == 1, "%s is implemented for single-context meshes", who);
  PPH_REQUIRE(ctx, n_dense >= 0 && m >= 0, "%s: negative count", who);
  PPH_REQUIRE(ctx, n_outside && (n_dense == 0 || dense) && (m == 0 || (x && field)), "%s: NULL buffer with a non-zero count", who);
  PPH_REQUIRE(ctx, n_dense <= SRC_MAX_DENSE, "%s: at most %d dense loads, got %lld", who, SRC_MAX_DENSE, (long long)n_dense);
  PPH_REQUIRE(ctx, m < ((int64_t)1 << 31) / 32, "%s: too many points (%lld)", who, (long long)m);
  PPH_REQUIRE(ctx, tol >= 0.0 && tol < 0.5, "%s: tol must be in [0, 0.5) box-local units", who);
  for (int64_t p = 0; p < m; ++p)
    PPH_REQUIRE(ctx, field[p] == 0 || field[p] == 1, "%s: field[%lld] = %d, the networks are 0 and 1", who, (long long)p, (int)field[p]);
  return PPH_OK;
}

// the point rows of `ns` (kernel, one fetch) and their by-dof CSR (host, one upload); x on the device
static int src_build_points(pph_ctx* ctx, SourceSet& ns, const double* x_dev, const int32_t* field_host, double tol,
                            DevBuf<int32_t>& fld) {
  const MeshData& ms = ctx->mesh;
  const int64_t m = ns.m;
  const int nb = ns.nb;
  const size_t ne = (size_t)m * nb;
  PPH_TRY(ns.pt_dof.alloc(ctx, ne));
  PPH_TRY(ns.pt_w.alloc(ctx, ne));
  PPH_TRY(fld.alloc(ctx, (size_t)m));
  PPH_HIP(ctx, hipMemcpyAsync(fld.p, field_host, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
  EvalGeo g;
  g.n[0] = ms.nx; g.n[1] = ms.ny; g.n[2] = (ms.dim == 3) ? ms.nzl : 1;
  if (ms.kind == PPH_CELL_QUAD) src_rows_launch<PPH_CELL_QUAD>(ctx, x_dev, fld.p, m, g, tol, ns.pt_dof.p, ns.pt_w.p);
  else if (ms.kind == PPH_CELL_TRI) src_rows_launch<PPH_CELL_TRI>(ctx, x_dev, fld.p, m, g, tol, ns.pt_dof.p, ns.pt_w.p);
  else if (ms.kind == PPH_CELL_HEX) src_rows_launch<PPH_CELL_HEX>(ctx, x_dev, fld.p, m, g, tol, ns.pt_dof.p, ns.pt_w.p);
  else src_rows_launch<PPH_CELL_TET>(ctx, x_dev, fld.p, m, g, tol, ns.pt_dof.p, ns.pt_w.p);
  PPH_HIP(ctx, hipGetLastError());
  std::vector<int64_t> dof(ne);
  std::vector<double> val(ne);
  PPH_HIP(ctx, hipMemcpyAsync(dof.data(), ns.pt_dof.p, sizeof(int64_t) * ne, hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipMemcpyAsync(val.data(), ns.pt_w.p, sizeof(double) * ne, hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // regroup by dof: the entries are generated in point order, so a stable sort by dof leaves every row in point order
  std::vector<int64_t> order;
  order.reserve(ne);
  ns.n_outside = 0;
  for (int64_t p = 0; p < m; ++p) {
    if (dof[(size_t)p * nb] < 0) { ++ns.n_outside; continue; }
    for (int b = 0; b < nb; ++b) order.push_back(p * nb + b);
  }
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return dof[(size_t)a] < dof[(size_t)b]; });
  std::vector<int64_t> rowptr(1, 0), row_dof;
  std::vector<int32_t> ent_pt(order.size());
  std::vector<double> ent_w(order.size());
  const int64_t N = 2 * ctx->n;
  for (size_t e = 0; e < order.size(); ++e) {
    const int64_t d = dof[(size_t)order[e]];
    PPH_REQUIRE(ctx, d >= 0 && d < N, "pph_sources_set: the point kernel returned the dof %lld outside [0, %lld)", (long long)d, (long long)N);
    if (row_dof.empty() || row_dof.back() != d) {
      if (!row_dof.empty()) rowptr.push_back((int64_t)e);
      row_dof.push_back(d);
    }
    ent_pt[e] = (int32_t)(order[e] / nb);
    ent_w[e] = val[(size_t)order[e]];
  }
  if (!row_dof.empty()) rowptr.push_back((int64_t)order.size());
  ns.n_touched = (int64_t)row_dof.size();
  if (ns.n_touched > 0) {
    PPH_TRY(ns.rowptr.alloc(ctx, rowptr.size()));
    PPH_TRY(ns.row_dof.alloc(ctx, row_dof.size()));
    PPH_TRY(ns.ent_pt.alloc(ctx, ent_pt.size()));
    PPH_TRY(ns.ent_w.alloc(ctx, ent_w.size()));
    PPH_HIP(ctx, hipMemcpyAsync(ns.rowptr.p, rowptr.data(), sizeof(int64_t) * rowptr.size(), hipMemcpyHostToDevice, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(ns.row_dof.p, row_dof.data(), sizeof(int64_t) * row_dof.size(), hipMemcpyHostToDevice, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(ns.ent_pt.p, ent_pt.data(), sizeof(int32_t) * ent_pt.size(), hipMemcpyHostToDevice, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(ns.ent_w.p, ent_w.data(), sizeof(double) * ent_w.size(), hipMemcpyHostToDevice, ctx->stream));
    PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the host vectors go out of scope)
  }
  return PPH_OK;
}

// builds the new set beside the old one: a failed call leaves the context's set as it was
static int src_set(pph_ctx* ctx, const double* dense, int64_t n_dense, const double* x, const int32_t* field, int64_t m, double tol,
                   int64_t* n_outside, bool on_device) {
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const MeshData& ms = ctx->mesh;
  const size_t N = 2 * (size_t)ctx->n;
  SourceSet ns;
  DevBuf<double> xb;
  DevBuf<int32_t> fld;
  auto build = [&]() -> int {
    ns.n_dense = n_dense; ns.m = m; ns.nb = src_nb(ms);
    if (n_dense > 0) {
      PPH_TRY(ns.dense.alloc(ctx, (size_t)n_dense * N));
      PPH_HIP(ctx, hipMemcpyAsync(ns.dense.p, dense, sizeof(double) * (size_t)n_dense * N,
                                  on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    }
    if (m > 0) {
      const double* xd = x;
      if (!on_device) {
        PPH_TRY(xb.alloc(ctx, (size_t)m * ms.dim));
        PPH_HIP(ctx, hipMemcpyAsync(xb.p, x, sizeof(double) * (size_t)m * ms.dim, hipMemcpyHostToDevice, ctx->stream));
        xd = xb.p;
      }
      PPH_TRY(src_build_points(ctx, ns, xd, field, tol, fld));
    }
    PPH_TRY(ns.coef.alloc(ctx, (size_t)(n_dense + m)));
    PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the caller's arrays are free again)
    return PPH_OK;
  };
  const int st = build();
  if (st < 0) (void)hipStreamSynchronize(ctx->stream);
  xb.release(); fld.release();
  if (st < 0) { ns.release(); return st; }
  ctx->src.release();
  ctx->src = ns;   // (DevBuf holds plain pointers: the context owns the allocations from here on)
  ctx->src.on = true;
  *n_outside = ns.n_outside;
  return PPH_OK;
}

extern "C" int pph_sources_set(pph_ctx* ctx, const double* dense_host, int64_t n_dense, const double* x_host, const int32_t* field,
                               int64_t m, double tol, int64_t* n_outside) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(src_set_check(ctx, "pph_sources_set", dense_host, n_dense, x_host, field, m, tol, n_outside));
  return src_set(ctx, dense_host, n_dense, x_host, field, m, tol, n_outside, false);
}

extern "C" int pph_sources_set_device(pph_ctx* ctx, const double* dense_dev, int64_t n_dense, const double* x_dev,
                                      const int32_t* field, int64_t m, double tol, int64_t* n_outside) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(src_set_check(ctx, "pph_sources_set_device", dense_dev, n_dense, x_dev, field, m, tol, n_outside));
  return src_set(ctx, dense_dev, n_dense, x_dev, field, m, tol, n_outside, true);
}

extern "C" int pph_sources_clear(pph_ctx* ctx) {
  if (!ctx) return PPH_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  ctx->src.release();
  return PPH_OK;
}

extern "C" int pph_sources_count(pph_ctx* ctx, int64_t* count) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, count != nullptr, "pph_sources_count: NULL buffer");
  *count = ctx->src.on ? ctx->src.count() : -1;
  return PPH_OK;
}

static int src_apply_check(pph_ctx* ctx, const char* who, const double* coef, const double* b) {
  PPH_REQUIRE(ctx, ctx->mesh_ok, "%s before pph_mesh_build", who);
  PPH_REQUIRE(ctx, ctx->world == 1, "%s is implemented for single-context meshes", who);
  PPH_REQUIRE(ctx, ctx->src.on, "%s: the context holds no source set (pph_sources_set)", who);
  PPH_REQUIRE(ctx, b != nullptr && (coef != nullptr || ctx->src.count() == 0), "%s: NULL buffer", who);
  return PPH_OK;
}

// uploads the coefficient row and enqueues the kernels on b (device)
static int src_apply_dev(pph_ctx* ctx, const double* coef_host, double* b) {
  const int64_t K = ctx->src.count();
  if (K == 0) return PPH_OK;
  PPH_HIP(ctx, hipMemcpyAsync(ctx->src.coef.p, coef_host, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, ctx->stream));
  return src_apply_launch(ctx, ctx->src.coef.p, b);
}

extern "C" int pph_sources_apply_device(pph_ctx* ctx, const double* coef, double* b_dev) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(src_apply_check(ctx, "pph_sources_apply_device", coef, b_dev));
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const int st = src_apply_dev(ctx, coef, b_dev);
  const hipError_t e = hipStreamSynchronize(ctx->stream);   // (the caller's arrays are free again when the call returns)
  if (st < 0) return st;
  PPH_HIP(ctx, e);
  return PPH_OK;
}

extern "C" int pph_sources_apply(pph_ctx* ctx, const double* coef, double* b_host) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(src_apply_check(ctx, "pph_sources_apply", coef, b_host));
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = 2 * (size_t)ctx->n;
  DevBuf<double> b;
  PPH_TRY(b.alloc(ctx, N));
  int st = PPH_OK;
  hipError_t e = hipMemcpyAsync(b.p, b_host, sizeof(double) * N, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    st = src_apply_dev(ctx, coef, b.p);
    if (st == PPH_OK) e = hipMemcpyAsync(b_host, b.p, sizeof(double) * N, hipMemcpyDeviceToHost, ctx->stream);
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  b.release();
  if (st < 0) return st;
  if (e != hipSuccess) {
    pph_set_error(ctx, "pph_sources_apply: copy failed: %s", hipGetErrorString(e));
    return PPH_ERR_HIP;
  }
  return PPH_OK;
}
