// Coupled multigrid (PPH_PC_CMG): one symmetric V-cycle on the monolithic 2n x 2n system
//   A_l = [[A11_l, C_l], [C_l^T, A22_l]],   C_l = -(beta/mu) F0 M_l F1
// over the CG-1 hierarchy of pph_mg.hip (same levels, same rediscretised diagonal blocks, same injected masks, the scalar
// transfers applied per field).  What is new is the smoother: Chebyshev on [lam_l / 4, lam_l] with the inverse of the
// 2 x 2 block of the two pressures of one node in place of 1 / diag, so that the zeroth-order exchange term - which the
// sweeps of the split solvers have to iterate out - is resolved pointwise on every level.  lam_l is the largest absolute
// row sum of D_l^-1 A_l.  Coarsest level: CG on A_L under D_L^-1 to rtol 1e-12.
//
// The hot path is k_cmg_row: after the two diagonal-block products t = (A11 d1 | A22 d2), which run in the library's product
// routines (row dictionary / stencil-ELL / CSR, whatever the level has), ONE pass over the rows walks the mass-matrix row
// once for both fields - (M d2)_i and (M d1)_i from one read of the row - and finishes the step for both dofs of node i
// in registers: residual update, 2 x 2 inverse, Chebyshev recurrence, x += d'.  G lanes per row (8 for the 27- and
// 15-entry rows of hexahedra and tetrahedra, 4 for the 9 and 7 of 2D), partial sums added by a shuffle tree in a fixed
// order: no atomics, two applications give the same bits.  Column masks are not needed in the walk: every vector the cycle
// forms is 0 on the constrained dofs of its field (the input is masked, the blocks of such nodes are diagonal, the
// transfers are masked), so F1 d2 = d2.
//
// Bytes per row of a smoothing step (hexahedra, interior): M row 27 x (8 + 4) + 8 of row pointer, t 16, r 32, blocks 32,
// d 16 (the gathers of neighbouring d are served by the caches), d' 16, x 32, masks 2 = 478 B (cmg_step_bytes); the two
// products before it move 2 x (2 .. 120) B of operator per row plus their vectors.
#include "pph_internal.h"
#include <chrono>
#include <cmath>
#include <cstring>
#include <utility>

#define CMG_CHEB_LOWER 0.25
#define CMG_GRID_BLOCKS 2048          // grid cap of the row kernels (256 threads each): more rows than fit make a lane loop
#define CMG_NODE_BLOCKS 1024          // ... of the one-thread-per-node kernels (k_cmg_init, k_cmg_mask_copy)
#define CMG_COARSE_ONCHIP 4096        // coarsest levels of at most this many nodes are solved inside one workgroup
enum { CMG_S = 40 };                  // reduction slots of the host-driven coarsest solve (ctx->scal)

static inline int cmg_lanes(const pph_ctx* ctx) { return ctx->mesh.dim == 3 ? 8 : 4; }
static inline int cmg_grid(int64_t n, int lanes) {
  int64_t b = ceil_div64(n * lanes, 256);
  if (b < 1) b = 1;
  if (b > CMG_GRID_BLOCKS) b = CMG_GRID_BLOCKS;
  return (int)b;
}
static inline int cmg_grid1(int64_t n) {
  const int64_t b = ceil_div64(n, 256);
  return (int)(b < 1 ? 1 : (b > CMG_NODE_BLOCKS ? CMG_NODE_BLOCKS : b));
}
static inline MeshData& cmg_mesh(pph_ctx* ctx, int l) { return l == 0 ? ctx->mesh : ctx->mg[l].mesh; }

// sum over the G lanes of a row group, every lane receives it (butterfly: a fixed order)
template <int G>
__device__ __forceinline__ double cmg_group_sum(double v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}

// ---- set-up of one level: inverted node blocks, the bound lam, (coarsest level) the four operators as CSR values ----------
// Block of node i: [[d11, d12], [d12, d22]], d11 = a K_ii + b M_ii, d22 = c K_ii + b M_ii, d12 = -b M_ii; a constrained field
// has the unit row of the eliminated operator and no coupling.  Its determinant d11 d22 - d12^2 cancels when b M_ii
// dominates; with s1 = d11 + d12, s2 = d22 + d12 (the stiffness parts) it is s1 s2 - d12 (s1 + s2), all terms >= 0.
template <int G>
__global__ __launch_bounds__(256) void k_cmg_setup(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                   const double* __restrict__ K, const double* __restrict__ M, int64_t n,
                                                   double a, double b, double c, double b1, double b2,
                                                   const uint8_t* __restrict__ m0,
                                                   const uint8_t* __restrict__ m1, double* __restrict__ binv,
                                                   unsigned long long* __restrict__ lam, double* __restrict__ v11,
                                                   double* __restrict__ v22, double* __restrict__ v12,
                                                   double* __restrict__ v21) {
  const int sub = threadIdx.x % G;
  const double cb = -b;
  double best = 0.0;
  for (int64_t row = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / G; row < n;
       row += ((int64_t)gridDim.x * blockDim.x) / G) {
    const int64_t s0 = rowptr[row], e0 = rowptr[row + 1];
    double kd = 0.0, md = 0.0;
    for (int64_t k = s0 + sub; k < e0; k += G)
      if ((int64_t)col[k] == row) { kd = K[k]; md = M[k]; }
    kd = cmg_group_sum<G>(kd);
    md = cmg_group_sum<G>(md);
    const bool f0 = m0[row] != 0, f1 = m1[row] != 0;
    const double d11 = f0 ? 1.0 : a * kd + b1 * md;   // (b1, b2 = b + sigma_f: the diagonal blocks' mass coefficients;
    const double d22 = f1 ? 1.0 : c * kd + b2 * md;   //  s1 = d11 + d12 = a kd + sigma1 md >= 0 still holds, the coupling stays -b M)
    const double d12 = (f0 || f1) ? 0.0 : cb * md;
    const double s1 = d11 + d12, s2 = d22 + d12;
    const double det = s1 * s2 - d12 * (s1 + s2);
    const double i11 = d22 / det, i12 = -d12 / det, i22 = d11 / det;
    double sa = 0.0, sb = 0.0;
    for (int64_t k = s0 + sub; k < e0; k += G) {
      const int64_t j = col[k];
      const double kj = K[k], mj = M[k];
      const bool g0 = m0[j] != 0, g1 = m1[j] != 0;
      const double a11 = f0 ? (j == row ? 1.0 : 0.0) : (g0 ? 0.0 : a * kj + b1 * mj);
      const double a22 = f1 ? (j == row ? 1.0 : 0.0) : (g1 ? 0.0 : c * kj + b2 * mj);
      const double c12 = (f0 || g1) ? 0.0 : cb * mj;   // C_ij
      const double c21 = (f1 || g0) ? 0.0 : cb * mj;   // (C^T)_ij
      sa += fabs(i11 * a11 + i12 * c21) + fabs(i11 * c12 + i12 * a22);
      sb += fabs(i12 * a11 + i22 * c21) + fabs(i12 * c12 + i22 * a22);
      if (v11) { v11[k] = a11; v22[k] = a22; v12[k] = c12; v21[k] = c21; }
    }
    sa = cmg_group_sum<G>(sa);
    sb = cmg_group_sum<G>(sb);
    if (sub == 0) {
      binv[row] = i11; binv[n + row] = i12; binv[2 * n + row] = i12; binv[3 * n + row] = i22;
      const double s = sa > sb ? sa : sb;
      best = s > best ? s : best;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_down(best, o, 64);
    best = t > best ? t : best;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(lam, (unsigned long long)__double_as_longlong(best));
}

// ---- the row walk ---------------------------------------------------------------------------------------------------------
// s1 = cb (M v2)_i (0 where field 0 is constrained at i), s2 = cb (M v1)_i (0 where field 1 is), t = (A11 v1 | A22 v2), then
// MODE 0, smoothing step:  r -= t + s;  d' = c1 v + c2 D^-1 r;  x += d'      (d' to dnew: other rows still read v = d)
// MODE 1, residual:        r = b - t - s, 0 on constrained dofs
template <int G, int MODE>
__global__ __launch_bounds__(256) void k_cmg_row(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                 const double* __restrict__ M, int64_t n, double cb,
                                                 const double* __restrict__ v, const double* __restrict__ t,
                                                 const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1,
                                                 const double* __restrict__ binv, double* __restrict__ r,
                                                 double* __restrict__ dnew, double* __restrict__ x, double c1, double c2,
                                                 const double* __restrict__ b) {
  const int sub = threadIdx.x % G;
  for (int64_t row = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / G; row < n;
       row += ((int64_t)gridDim.x * blockDim.x) / G) {
    const int64_t s0 = rowptr[row], e0 = rowptr[row + 1];
    double a1 = 0.0, a2 = 0.0;
    for (int64_t k = s0 + sub; k < e0; k += G) {
      const int64_t j = col[k];
      const double m = M[k];
      a1 += m * v[n + j];
      a2 += m * v[j];
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
      a1 += __shfl_down(a1, o, G);
      a2 += __shfl_down(a2, o, G);
    }
    if (sub == 0) {
      const bool f0 = m0[row] != 0, f1 = m1[row] != 0;
      const double s1 = f0 ? 0.0 : cb * a1, s2 = f1 ? 0.0 : cb * a2;
      if (MODE == 0) {
        const double r1 = r[row] - t[row] - s1, r2 = r[n + row] - t[n + row] - s2;
        const double z1 = binv[row] * r1 + binv[n + row] * r2;
        const double z2 = binv[2 * n + row] * r1 + binv[3 * n + row] * r2;
        const double dn1 = c1 * v[row] + c2 * z1, dn2 = c1 * v[n + row] + c2 * z2;
        r[row] = r1; r[n + row] = r2;
        dnew[row] = dn1; dnew[n + row] = dn2;
        x[row] += dn1; x[n + row] += dn2;
      } else {
        r[row] = f0 ? 0.0 : b[row] - t[row] - s1;
        r[n + row] = f1 ? 0.0 : b[n + row] - t[n + row] - s2;
      }
    }
  }
}

// first Chebyshev step: d = D^-1 r / theta;  x = d (zero guess) or x += d
__global__ __launch_bounds__(256) void k_cmg_init(double* __restrict__ x, double* __restrict__ d, const double* __restrict__ r,
                                                  const double* __restrict__ binv, double inv_theta, int zero_guess,
                                                  int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double r1 = r[i], r2 = r[n + i];
    const double d1 = (binv[i] * r1 + binv[n + i] * r2) * inv_theta;
    const double d2 = (binv[2 * n + i] * r1 + binv[3 * n + i] * r2) * inv_theta;
    d[i] = d1; d[n + i] = d2;
    x[i] = zero_guess ? d1 : x[i] + d1;
    x[n + i] = zero_guess ? d2 : x[n + i] + d2;
  }
}

// out = in with the constrained entries of both fields set to 0
__global__ __launch_bounds__(256) void k_cmg_mask_copy(double* __restrict__ out, const double* __restrict__ in,
                                                       const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1,
                                                       int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    out[i] = m0[i] ? 0.0 : in[i];
    out[n + i] = m1[i] ? 0.0 : in[n + i];
  }
}

// ---- coarsest level ---------------------------------------------------------------------------------------------------
// q = A_L p from the four CSR value arrays of the set-up, one thread per node
__device__ __forceinline__ void cmg_coarse_row(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                               const double* __restrict__ v11, const double* __restrict__ v22,
                                               const double* __restrict__ v12, const double* __restrict__ v21,
                                               const double* __restrict__ p, int64_t n, int64_t i, double& q1, double& q2) {
  double s1 = 0.0, s2 = 0.0;
  for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
    const int64_t j = col[k];
    const double p1 = p[j], p2 = p[n + j];
    s1 += v11[k] * p1 + v12[k] * p2;
    s2 += v21[k] * p1 + v22[k] * p2;
  }
  q1 = s1; q2 = s2;
}

__global__ __launch_bounds__(256) void k_cmg_coarse_apply(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const double* __restrict__ v11, const double* __restrict__ v22,
                                                          const double* __restrict__ v12, const double* __restrict__ v21,
                                                          const double* __restrict__ p, double* __restrict__ q, int64_t n) {
  // one thread per node, as many workgroups as that takes (no loop: a coarsest level is small beside the fine one)
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) {
    double q1, q2;
    cmg_coarse_row(rowptr, col, v11, v22, v12, v21, p, n, i, q1, q2);
    q[i] = q1; q[n + i] = q2;
  }
}

__device__ __forceinline__ double cmg_block_sum(double v, double* lds) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += lds[w];
  return t;
}

// CG on A_L under D_L^-1 inside ONE workgroup (the recurrence and test of k_coarse_cg, pph_mg.hip: ||D^-1 r|| <= rtol
// ||D^-1 b||, zero guess).  rec[0] += 1 when the solve stops short of its tolerance (iteration limit, p.Ap <= 0 or NaN).
__global__ __launch_bounds__(1024) void k_cmg_coarse_cg(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const double* __restrict__ v11, const double* __restrict__ v22,
                                                        const double* __restrict__ v12, const double* __restrict__ v21,
                                                        const double* __restrict__ binv, const double* __restrict__ b,
                                                        double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
                                                        double* __restrict__ q, int n, double rtol, int max_it,
                                                        unsigned long long* __restrict__ rec) {
  __shared__ double lds[16];
  const int tid = threadIdx.x, nt = blockDim.x;
  double zz = 0.0, rz = 0.0;
  for (int i = tid; i < n; i += nt) {
    const double r1 = b[i], r2 = b[n + i];
    const double z1 = binv[i] * r1 + binv[n + i] * r2, z2 = binv[2 * n + i] * r1 + binv[3 * n + i] * r2;
    x[i] = 0.0; x[n + i] = 0.0;
    r[i] = r1; r[n + i] = r2;
    p[i] = z1; p[n + i] = z2;
    zz += z1 * z1 + z2 * z2; rz += r1 * z1 + r2 * z2;
  }
  zz = cmg_block_sum(zz, lds);
  rz = cmg_block_sum(rz, lds);
  const double tol = rtol * sqrt(zz);
  if (!(sqrt(zz) > tol)) { if (tid == 0 && !(zz == 0.0)) rec[0] += 1ull; return; }   // zero right-hand side: x = 0
  for (int it = 0; it < max_it; ++it) {
    __syncthreads();   // p complete
    double pq = 0.0;
    for (int i = tid; i < n; i += nt) {
      double q1, q2;
      cmg_coarse_row(rowptr, col, v11, v22, v12, v21, p, n, i, q1, q2);
      q[i] = q1; q[n + i] = q2;
      pq += p[i] * q1 + p[n + i] * q2;
    }
    pq = cmg_block_sum(pq, lds);
    if (!(pq > 0.0)) { if (tid == 0) rec[0] += 1ull; return; }
    const double alpha = rz / pq;
    double zz2 = 0.0, rz2 = 0.0;
    for (int i = tid; i < n; i += nt) {
      x[i] += alpha * p[i]; x[n + i] += alpha * p[n + i];
      const double r1 = r[i] - alpha * q[i], r2 = r[n + i] - alpha * q[n + i];
      const double z1 = binv[i] * r1 + binv[n + i] * r2, z2 = binv[2 * n + i] * r1 + binv[3 * n + i] * r2;
      r[i] = r1; r[n + i] = r2;
      q[i] = z1; q[n + i] = z2;   // (q is free until the next product: keeps z for the direction update)
      zz2 += z1 * z1 + z2 * z2; rz2 += r1 * z1 + r2 * z2;
    }
    zz2 = cmg_block_sum(zz2, lds);
    rz2 = cmg_block_sum(rz2, lds);
    if (sqrt(zz2) <= tol) return;
    const double beta = rz2 / rz;
    __syncthreads();   // every thread has read p[col] of this iteration's product
    for (int i = tid; i < n; i += nt) {
      p[i] = q[i] + beta * p[i];
      p[n + i] = q[n + i] + beta * p[n + i];
    }
    rz = rz2;
  }
  if (tid == 0) rec[0] += 1ull;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
void cmg_release(pph_ctx* ctx) {
  for (CmgLevel& C : ctx->cmg) {
    C.K.release(); C.M.release(); C.km_ok = false; C.Kp = C.Mp = nullptr;
    C.binv.release(); C.x.release(); C.b.release(); C.r.release(); C.d.release(); C.e.release(); C.t.release();
    for (DevBuf<double>& v : C.cval) v.release();
  }
  ctx->cmg.clear();
  ctx->cmg_lam.release();
  ctx->cmg_rec.release();
  ctx->cmg_ok = false;
}

#define CMG_SETUP_GO(GG)                                                                                                   \
  hipLaunchKernelGGL(k_cmg_setup<GG>, dim3(cmg_grid(n, GG)), dim3(256), 0, ctx->stream, m.rowptr.p, m.col.p, C.Kp, C.Mp, n, \
                     ctx->a, ctx->b, ctx->c, ctx->bm(0), ctx->bm(1), L.maskp[0], L.maskp[1], C.binv.p, ctx->cmg_lam.p + l, v[0], v[1], v[2], v[3])

int cmg_setup(pph_ctx* ctx) {
  PPH_REQUIRE(ctx, ctx->world == 1, "pc_type pph_cmg: single context only (no slab decomposition)");
  PPH_REQUIRE(ctx, ctx->mesh.degree == 1, "pc_type pph_cmg: the coupled cycle runs on the CG-1 hierarchy; degree-2 spaces have none");
  PPH_TRY(mg_setup(ctx));
  if (ctx->cmg_ok && ctx->cmg_epoch == ctx->mg_values_epoch) return PPH_OK;
  const int nlev = (int)ctx->mg.size();
  if ((int)ctx->cmg.size() != nlev) { cmg_release(ctx); ctx->cmg.resize((size_t)nlev); }
  if (!ctx->cmg_lam.p) PPH_TRY(ctx->cmg_lam.alloc(ctx, 32));
  if (!ctx->cmg_rec.p) {
    PPH_TRY(ctx->cmg_rec.alloc(ctx, 1));
    PPH_HIP(ctx, hipMemsetAsync(ctx->cmg_rec.p, 0, sizeof(unsigned long long), ctx->stream));
  }
  PPH_HIP(ctx, hipMemsetAsync(ctx->cmg_lam.p, 0, 32 * sizeof(unsigned long long), ctx->stream));
  const int G = cmg_lanes(ctx);
  for (int l = 0; l < nlev; ++l) {
    MgLevel& L = ctx->mg[l];
    CmgLevel& C = ctx->cmg[(size_t)l];
    MeshData& m = cmg_mesh(ctx, l);
    const int64_t n = L.n;
    // K and M of the level's mesh as CSR values: they depend on the mesh only and are kept with the level while the
    // hierarchy stands.  They are the cycle's own: a mesh whose K and M count as valid is assembled from them from then
    // on (pph_assemble_dpp), and a context must assemble as it did before it ran a coupled cycle
    // (a mesh that holds valid K and M of its own - a level of the non-fused hierarchy, option asm_keep_km, after a Darcy
    // projection - lends them: no second copy)
    if (m.km_valid) {
      C.Kp = m.K.p; C.Mp = m.M.p;
    } else {
      if (!C.km_ok) {
        PPH_TRY(pph_launch_assemble_KM(ctx, m));
        std::swap(C.K, m.K);
        std::swap(C.M, m.M);
        m.K.release(); m.M.release();
        m.erows.release();   // (the two-pass assembly's element rows: scratch)
        C.km_ok = true;
      }
      C.Kp = C.K.p; C.Mp = C.M.p;
    }
    PPH_TRY(C.binv.alloc(ctx, (size_t)(4 * n)));
    PPH_TRY(C.r.alloc(ctx, (size_t)(2 * n)));
    PPH_TRY(C.d.alloc(ctx, (size_t)(2 * n)));
    PPH_TRY(C.e.alloc(ctx, (size_t)(2 * n)));
    PPH_TRY(C.t.alloc(ctx, (size_t)(2 * n)));
    PPH_TRY(C.b.alloc(ctx, (size_t)(2 * n)));
    if (l > 0) PPH_TRY(C.x.alloc(ctx, (size_t)(2 * n)));
    double* v[4] = {nullptr, nullptr, nullptr, nullptr};
    if (l == nlev - 1 && nlev > 1) {
      for (int q = 0; q < 4; ++q) { PPH_TRY(C.cval[q].alloc(ctx, (size_t)m.nnzb)); v[q] = C.cval[q].p; }
    }
    if (G == 8) CMG_SETUP_GO(8); else CMG_SETUP_GO(4);
  }
  unsigned long long bits[32];
  PPH_HIP(ctx, hipMemcpyAsync(bits, ctx->cmg_lam.p, sizeof(unsigned long long) * (size_t)nlev, hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  PPH_HIP(ctx, hipGetLastError());
  for (int l = 0; l < nlev; ++l) {
    double lam;
    memcpy(&lam, &bits[l], sizeof(double));
    PPH_REQUIRE(ctx, lam > 0.0 && lam == lam && std::isfinite(lam), "coupled multigrid level %d: bad spectral bound %g", l, lam);
    ctx->cmg[(size_t)l].lam = lam;
  }
  ctx->cmg_epoch = ctx->mg_values_epoch;
  ctx->cmg_ok = true;
  return PPH_OK;
}

// t = (A11_l v1 | A22_l v2): the library's products on the level's diagonal blocks
static void cmg_diag_products(pph_ctx* ctx, int l, const double* v, double* t) {
  const int64_t n = ctx->mg[l].n;
  for (int f = 0; f < 2; ++f) la_spmv(ctx, mg_level_csr(ctx, l, f), v + f * n, t + f * n);
}

#define CMG_ROW_GO(GG, MODE)                                                                                                  \
  hipLaunchKernelGGL((k_cmg_row<GG, MODE>), dim3(cmg_grid(n, GG)), dim3(256), 0, ctx->stream, m.rowptr.p, m.col.p, C.Mp, n, \
                     -ctx->b, v, t, L.maskp[0], L.maskp[1], C.binv.p, r, dnew, x, c1, c2, b)

// MODE as k_cmg_row; t must hold the diagonal-block products of v
static void cmg_row(pph_ctx* ctx, int l, int mode, const double* v, const double* t, double* r, double* dnew, double* x,
                    double c1, double c2, const double* b) {
  const MgLevel& L = ctx->mg[l];
  const CmgLevel& C = ctx->cmg[(size_t)l];
  const MeshData& m = cmg_mesh(ctx, l);
  const int64_t n = L.n;
  if (cmg_lanes(ctx) == 8) {
    if (mode == 0) CMG_ROW_GO(8, 0); else CMG_ROW_GO(8, 1);
  } else {
    if (mode == 0) CMG_ROW_GO(4, 0); else CMG_ROW_GO(4, 1);
  }
}

// algorithmic bytes of one fine-level smoothing pass of k_cmg_row: M's row (values, columns, row pointer) and the vectors
// and blocks of the epilogue; the gathers of d are not counted (neighbouring rows share them through the caches)
double cmg_step_bytes(const pph_ctx* ctx) {
  return 12.0 * (double)ctx->nnzb + (double)ctx->n * (8.0 + 16.0 /* t */ + 32.0 /* r */ + 32.0 /* blocks */ + 16.0 /* d */ +
                                                   16.0 /* d' */ + 32.0 /* x */ + 2.0 /* masks */);
}

// r = b - A_l x, 0 on constrained dofs
static void cmg_resid(pph_ctx* ctx, int l, const double* x, const double* b, double* r) {
  CmgLevel& C = ctx->cmg[(size_t)l];
  cmg_diag_products(ctx, l, x, C.t.p);
  cmg_row(ctx, l, 1, x, C.t.p, r, nullptr, nullptr, 0.0, 0.0, b);
}

// `steps` Chebyshev steps under D^-1 on A_l x = b (the recurrence of the scalar smoother, pph_mg.hip: chebyshev)
static void cmg_chebyshev(pph_ctx* ctx, int l, const double* b, double* x, int steps, bool zero_guess) {
  CmgLevel& C = ctx->cmg[(size_t)l];
  const int64_t n = ctx->mg[l].n;
  const double hi = C.lam, lo = CMG_CHEB_LOWER * hi;
  const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo);
  const double sigma = theta / delta;
  double rho = 1.0 / sigma;
  double* r = C.r.p;
  const double* r0 = r;
  if (zero_guess) {
    if (steps > 1) la_copy(ctx, r, b, 2 * n);   // the recurrence updates r in place
    else r0 = b;
  } else {
    cmg_resid(ctx, l, x, b, r);
  }
  double *dcur = C.d.p, *dnext = C.e.p;
  hipLaunchKernelGGL(k_cmg_init, dim3(cmg_grid1(n)), dim3(256), 0, ctx->stream, x, dcur, r0, C.binv.p, 1.0 / theta,
                     zero_guess ? 1 : 0, n);
  for (int s = 1; s < steps; ++s) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    cmg_diag_products(ctx, l, dcur, C.t.p);
    cmg_row(ctx, l, 0, dcur, C.t.p, r, dnext, x, rho_new * rho, 2.0 * rho_new / delta, nullptr);
    double* sw = dcur; dcur = dnext; dnext = sw;
    rho = rho_new;
  }
}

// host-driven CG of a coarsest level too large for one workgroup (a mesh whose cell counts stop halving early)
static int cmg_coarse_host(pph_ctx* ctx, int l, const double* b, double* x) {
  CmgLevel& C = ctx->cmg[(size_t)l];
  const MeshData& m = cmg_mesh(ctx, l);
  const int64_t n = ctx->mg[l].n, N = 2 * n;
  double *r = C.r.p, *z = C.d.p, *p = C.e.p, *q = C.t.p;
  la_set(ctx, x, 0.0, N);
  la_copy(ctx, r, b, N);
  la_block2_apply(ctx, z, C.binv.p, r, n);
  la_copy(ctx, p, z, N);
  la_dot2(ctx, r, z, z, N, CMG_S);
  PPH_TRY(la_fetch(ctx, CMG_S, 2));
  double rz = ctx->h_scal[CMG_S];
  const double z0 = std::sqrt(ctx->h_scal[CMG_S + 1]);
  const double tol = 1e-12 * z0;
  if (!(z0 > tol)) { if (!(z0 == 0.0)) ctx->coarse_failed++; return PPH_OK; }
  for (int it = 0; it < ctx->coarse_max_it; ++it) {
    hipLaunchKernelGGL(k_cmg_coarse_apply, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, ctx->stream, m.rowptr.p, m.col.p, C.cval[0].p,
                       C.cval[1].p, C.cval[2].p, C.cval[3].p, p, q, n);
    la_dot(ctx, p, q, N, CMG_S + 2);
    PPH_TRY(la_fetch(ctx, CMG_S + 2, 1));
    const double pq = ctx->h_scal[CMG_S + 2];
    if (!(pq > 0.0)) { ctx->coarse_failed++; return PPH_OK; }
    const double alpha = rz / pq;
    la_axpy(ctx, x, alpha, p, N);
    la_axpy(ctx, r, -alpha, q, N);
    la_block2_apply(ctx, z, C.binv.p, r, n);
    la_dot2(ctx, r, z, z, N, CMG_S);
    PPH_TRY(la_fetch(ctx, CMG_S, 2));
    const double rz2 = ctx->h_scal[CMG_S];
    if (std::sqrt(ctx->h_scal[CMG_S + 1]) <= tol) return PPH_OK;
    la_axpby(ctx, p, 1.0, z, rz2 / rz, N);
    rz = rz2;
  }
  ctx->coarse_failed++;
  return PPH_OK;
}

// z = B r: one coupled cycle.  Entries of r on constrained dofs are taken as 0; z is 0 there.
int cmg_apply(pph_ctx* ctx, const double* rin, double* zout, int nsmooth) {
  const int nlev = (int)ctx->mg.size();
  const int ns = nsmooth > 0 ? nsmooth : 2;
  {
    const MgLevel& L = ctx->mg[0];
    hipLaunchKernelGGL(k_cmg_mask_copy, dim3(cmg_grid1(L.n)), dim3(256), 0, ctx->stream, ctx->cmg[0].b.p, rin, L.maskp[0],
                       L.maskp[1], L.n);
  }
  if (nlev == 1) {
    // a mesh that cannot be coarsened: the Chebyshev polynomial alone, as the scalar rule has it
    cmg_chebyshev(ctx, 0, ctx->cmg[0].b.p, zout, ns > 2 ? ns : 2, true);
    return PPH_OK;
  }
  for (int l = 0; l < nlev - 1; ++l) {
    CmgLevel& C = ctx->cmg[(size_t)l];
    CmgLevel& Cc = ctx->cmg[(size_t)l + 1];
    double* x = (l == 0) ? zout : C.x.p;
    cmg_chebyshev(ctx, l, C.b.p, x, ns, true);
    cmg_resid(ctx, l, x, C.b.p, C.r.p);
    const int64_t nf = ctx->mg[l].n, nc = ctx->mg[l + 1].n;
    for (int f = 0; f < 2; ++f) mg_restrict_field(ctx, l, f, C.r.p + f * nf, Cc.b.p + f * nc);
  }
  {
    const int l = nlev - 1;
    CmgLevel& C = ctx->cmg[(size_t)l];
    const MeshData& m = cmg_mesh(ctx, l);
    const int64_t n = ctx->mg[l].n;
    if (n <= CMG_COARSE_ONCHIP && ctx->coarse_on_device)
      hipLaunchKernelGGL(k_cmg_coarse_cg, dim3(1), dim3(n <= 256 ? 256 : 1024), 0, ctx->stream, m.rowptr.p, m.col.p, C.cval[0].p,
                         C.cval[1].p, C.cval[2].p, C.cval[3].p, C.binv.p, C.b.p, C.x.p, C.r.p, C.d.p, C.t.p, (int)n, 1e-12,
                         ctx->coarse_max_it, ctx->cmg_rec.p);
    else
      PPH_TRY(cmg_coarse_host(ctx, l, C.b.p, C.x.p));
  }
  for (int l = nlev - 2; l >= 0; --l) {
    CmgLevel& C = ctx->cmg[(size_t)l];
    CmgLevel& Cc = ctx->cmg[(size_t)l + 1];
    double* x = (l == 0) ? zout : C.x.p;
    const int64_t nf = ctx->mg[l].n, nc = ctx->mg[l + 1].n;
    for (int f = 0; f < 2; ++f) mg_prolong_add_field(ctx, l, f, x + f * nf, Cc.x.p + f * nc);
    cmg_chebyshev(ctx, l, C.b.p, x, ns, false);
  }
  return PPH_OK;
}

// coarsest solves on the device that stopped short since the last call (synchronises)
int cmg_collect_failures(pph_ctx* ctx) {
  if (!ctx->cmg_rec.p) return PPH_OK;
  unsigned long long rec = 0;
  PPH_HIP(ctx, hipMemcpyAsync(&rec, ctx->cmg_rec.p, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipMemsetAsync(ctx->cmg_rec.p, 0, sizeof(rec), ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (rec) ctx->coarse_failed += (int)rec;
  return PPH_OK;
}

// ms per fine-level smoothing pass of the row-walk kernel alone (the diagonal-block products are not in it), on the vectors
// the last cycle left behind
int cmg_step_bench(pph_ctx* ctx, int reps, double* ms_out) {
  PPH_REQUIRE(ctx, ctx->cmg_ok && !ctx->cmg.empty(), "coupled multigrid not set up");
  CmgLevel& C = ctx->cmg[0];
  cmg_diag_products(ctx, 0, C.d.p, C.t.p);
  for (int i = 0; i < reps + 3; ++i) {
    if (i == 3) PPH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    cmg_row(ctx, 0, 0, C.d.p, C.t.p, C.r.p, C.e.p, C.b.p, 0.0, 0.0, nullptr);   // (c1 = c2 = 0: the vectors stay finite)
  }
  PPH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  PPH_HIP(ctx, hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  PPH_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *ms_out = (double)ms / reps;
  return PPH_OK;
}
