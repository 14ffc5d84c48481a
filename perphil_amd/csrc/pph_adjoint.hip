// Adjoint solves and parameter gradients: a solve of the assembled system for a caller's right-hand side, and the three
// bilinear forms that turn (adjoint, solution) into gradients.
//
// No reference counterpart: the reference (src/perphil/solvers/solver.py:30-76) solves for given parameters and stops there.
// The operator of dpp.py:95-132 is symmetric, so the adjoint of a functional J(p) solves the SAME eliminated system
// F A F lambda = F dJ/dp, and with the un-eliminated stiffness and mass matrices K and M
//   dJ/dk1 = -o0 / mu,  dJ/dk2 = -o1 / mu,  dJ/dbeta = -o2 / mu,  dJ/dmu = (k1 o0 + k2 o1 + beta o2) / mu^2
//   o0 = lambda1^T K p1 = int grad lambda1 . grad p1,   o1 = lambda2^T K p2,   o2 = (lambda1 - lambda2)^T M (p1 - p2)
//
//   pph_solve_rhs*      a wrapper around pph_solve_device: the CONTENTS of the context's right-hand side, lifting and solution
//                       are exchanged with saved copies (the addresses stay: captured graphs hold them), the existing solve runs
//                       on F b with a zero lifting, and everything is put back bit for bit.
//   k_dpp_bilinear      o0, o1, o2 in one matrix-free pass over the boxes of the mesh: four nodal fields and the dof map are read
//                       once, nothing of K or M is stored.
//
// Element forms (uniform boxes, node spacing 1 / n_e; pph_flux.hip states the geometry):
//   Q1 / Q2: K_e = |box| sum_d n_d^2 (S in direction d, Mm in the others), M_e = |box| Mm x Mm (x Mm), with the 1-D stiffness and
//     mass matrices on [0, 1]: Q1 S = [1 -1; -1 1], Mm = [2 1; 1 2] / 6; Q2 (nodes 0, 1/2, 1) S = [7 -8 1; -8 16 -8; 1 -8 7] / 3,
//     Mm = [4 2 -1; 2 16 2; -1 2 4] / 30.  Applied by sum factorisation to the p side (a 1-D matrix along one direction at a time),
//     then one dot product with the lambda side: no element matrix is formed.
//   P1 / P2: every sub-cell of a box has exactly one edge along each axis, so d/dx_d = n_d (derivative along that edge).  P1: the
//     edge difference, constant in the cell.  P2: the gradient is linear, and for two linear functions g, h on a simplex
//     int g h = |c| / ((D + 1)(D + 2)) (sum_r g_r sum_r h_r + sum_r g_r h_r) over the vertex values: the edge derivatives are
//     evaluated at the vertices.  Mass: P1 the same formula on the nodal values; P2 the exact table int phi_a phi_b / |c| from
//     the barycentric integrals int prod lambda_i^a_i = |c| D! prod a_i! / (D + sum a_i)! (formed on the host, a kernel argument).
//
// Registers: 8 (Q1 hexahedra) x 4 fields are 32 doubles, held at once.  27 (Q2 hexahedra) x 4 would be 108 doubles before any
// work: there the three forms run one after the other on ONE pair (lambda side, p side) each - (lambda1, p1), (lambda2, p2),
// (lambda1 - lambda2, p1 - p2) - so that at most two gathered 27-vectors and the intermediates of the sum factorisation are
// live; the third form loads the four fields a second time, from cache (the lines were fetched by the first two).
//
// Determinism: k_integrate's layout.  A thread adds its boxes in grid-stride order, a workgroup its threads in a fixed LDS tree,
// k_bilinear_sum the workgroups' partial sums in a fixed order; the grid is a function of the mesh alone.  No atomics.
#include "pph_internal.h"
#include "pph_p2.h"
#include "pph_bilinear.h"   // BlGeo, BlTab, BlCell, bl_stiff, bl_mass, k_bilinear_sum, bl_p2_mass_table

// part[q * BL_MAX_BLOCKS + block]: this workgroup's share of o_q; lam, p: 2 n values, field-major
template <int KIND, int DEG>
__global__ __launch_bounds__(256, (BlCell<KIND, DEG>::ONE_PASS ? 1 : 2)) void k_dpp_bilinear(const int32_t* __restrict__ cells, const double* __restrict__ lam,
                                                      const double* __restrict__ p, int64_t n, int64_t nbox, BlGeo g, BlTab tab,
                                                      double* __restrict__ part) {
  using C = BlCell<KIND, DEG>;
  constexpr int NB = C::NB;
  __shared__ double lds[256];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t box = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; box < nbox; box += (int64_t)gridDim.x * blockDim.x) {
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int sub = 0; sub < C::CPB; ++sub) {
      const int32_t* cn = cells + (box * C::CPB + sub) * NB;
      int32_t id[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) id[k] = cn[k];
      if constexpr (C::ONE_PASS) {
        double l1[NB], l2[NB], q1[NB], q2[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) { l1[k] = lam[id[k]]; l2[k] = lam[n + id[k]]; q1[k] = p[id[k]]; q2[k] = p[n + id[k]]; }
        s[0] += bl_stiff<KIND, DEG>([&](int k) { return l1[k]; }, [&](int k) { return q1[k]; }, g, sub);
        s[1] += bl_stiff<KIND, DEG>([&](int k) { return l2[k]; }, [&](int k) { return q2[k]; }, g, sub);
        s[2] += bl_mass<KIND, DEG>([&](int k) { return l1[k] - l2[k]; }, [&](int k) { return q1[k] - q2[k]; }, g, tab);
      } else {
        // one form at a time, each value gathered where the form uses it (the scheduling barriers keep the next form's
        // gathers from being hoisted over this one's work)
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          s[f] += bl_stiff<KIND, DEG>([&](int k) { return lam[f * n + id[k]]; }, [&](int k) { return p[f * n + id[k]]; }, g, sub);
          __builtin_amdgcn_sched_barrier(0);
        }
        // (the same addresses again: behind an opaque copy of the pointers the loads are issued again instead of their
        // first results being kept alive across the two forms above)
        const double *lam3 = lam, *p3 = p;
        asm volatile("" : "+s"(lam3), "+s"(p3));
        s[2] += bl_mass<KIND, DEG>([&](int k) { return lam3[id[k]] - lam3[n + id[k]]; },
                                   [&](int k) { return p3[id[k]] - p3[n + id[k]]; }, g, tab);
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q] += s[q];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double t = bl_block_sum(acc[q], lds);
    if (threadIdx.x == 0) part[(int64_t)q * BL_MAX_BLOCKS + blockIdx.x] = t;
  }
}

static int bl_check(pph_ctx* ctx, const char* who, bool buffers) {
  PPH_REQUIRE(ctx, ctx->mesh_ok, "%s before pph_mesh_build", who);
  PPH_REQUIRE(ctx, ctx->world == 1, "%s is implemented for single-context meshes", who);
  PPH_REQUIRE(ctx, buffers, "%s: NULL buffer", who);
  return PPH_OK;
}

template <int KIND>
static void bl_launch(pph_ctx* ctx, int degree, int grid, const double* lam, const double* p, int64_t nbox, const BlGeo& g,
                      const BlTab& tab, double* part) {
  const int32_t* cells = ctx->mesh.cells.p;
  if (degree == 2)
    hipLaunchKernelGGL((k_dpp_bilinear<KIND, 2>), dim3(grid), dim3(256), 0, ctx->stream, cells, lam, p, ctx->mesh.n, nbox, g, tab, part);
  else
    hipLaunchKernelGGL((k_dpp_bilinear<KIND, 1>), dim3(grid), dim3(256), 0, ctx->stream, cells, lam, p, ctx->mesh.n, nbox, g, tab, part);
}

// the results reach the host through `part` (released by the entry point whichever way the call ends)
static int bilinear_dev(pph_ctx* ctx, DevBuf<double>& part, const double* lam, const double* p, double* out3) {
  const MeshData& m = ctx->mesh;
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const int nd[3] = {m.nx, m.ny, (m.dim == 3) ? m.nzl : 1};
  const int64_t nbox = (int64_t)nd[0] * nd[1] * nd[2];
  const int cpb = p2_cells_per_box(m.kind);
  BlGeo g;
  g.vol = 1.0 / ((double)nbox * (double)cpb);
  for (int d = 0; d < 3; ++d) g.cd[d] = (d < m.dim) ? (double)nd[d] * (double)nd[d] * g.vol : 0.0;
  BlTab tab;
  bl_p2_mass_table(m.dim, &tab);
  PPH_TRY(part.alloc(ctx, (size_t)3 * BL_MAX_BLOCKS + 3));
  double* res = part.p + (size_t)3 * BL_MAX_BLOCKS;
  const int64_t nb = ceil_div64(nbox, 256);
  const int grid = (int)(nb < 1 ? 1 : (nb < BL_MAX_BLOCKS ? nb : BL_MAX_BLOCKS));
  if (m.kind == PPH_CELL_QUAD) bl_launch<PPH_CELL_QUAD>(ctx, m.degree, grid, lam, p, nbox, g, tab, part.p);
  else if (m.kind == PPH_CELL_TRI) bl_launch<PPH_CELL_TRI>(ctx, m.degree, grid, lam, p, nbox, g, tab, part.p);
  else if (m.kind == PPH_CELL_HEX) bl_launch<PPH_CELL_HEX>(ctx, m.degree, grid, lam, p, nbox, g, tab, part.p);
  else bl_launch<PPH_CELL_TET>(ctx, m.degree, grid, lam, p, nbox, g, tab, part.p);
  hipLaunchKernelGGL(k_bilinear_sum, dim3(3), dim3(256), 0, ctx->stream, part.p, grid, res);
  PPH_HIP(ctx, hipGetLastError());
  PPH_HIP(ctx, hipMemcpyAsync(out3, res, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PPH_OK;
}

extern "C" int pph_dpp_bilinear_device(pph_ctx* ctx, const double* lam_dev, const double* p_dev, double* out) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(bl_check(ctx, "pph_dpp_bilinear_device", lam_dev && p_dev && out));
  DevBuf<double> part;
  const int st = bilinear_dev(ctx, part, lam_dev, p_dev, out);
  part.release();
  return st;
}

extern "C" int pph_dpp_bilinear(pph_ctx* ctx, const double* lam_host, const double* p_host, double* out) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(bl_check(ctx, "pph_dpp_bilinear", lam_host && p_host && out));
  const size_t n2 = 2 * (size_t)ctx->mesh.n;
  DevBuf<double> lam, p, part;
  int st = PPH_OK;
  auto upload = [&](DevBuf<double>& d, const double* host) -> int {
    PPH_HIP(ctx, hipSetDevice(ctx->device));
    PPH_TRY(d.alloc(ctx, n2));
    PPH_HIP(ctx, hipMemcpyAsync(d.p, host, sizeof(double) * n2, hipMemcpyHostToDevice, ctx->stream));
    return PPH_OK;
  };
  st = upload(lam, lam_host);
  if (st == PPH_OK) st = upload(p, p_host);
  if (st == PPH_OK) st = bilinear_dev(ctx, part, lam.p, p.p, out);
  else (void)hipStreamSynchronize(ctx->stream);   // (a copy may still read the caller's array)
  lam.release(); p.release(); part.release();
  return st;
}

// ---- solve for a caller's right-hand side --------------------------------------------------------------------------------
// dst = (mask != 0) ? 0 : src over both fields (n entries each, one mask per field)
__global__ __launch_bounds__(256) void k_mask_free(double* __restrict__ dst, const double* __restrict__ src,
                                                   const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 2 * n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t m = (i < n) ? m0[i] : m1[i - n];
    dst[i] = m ? 0.0 : src[i];
  }
}

// the exchange, the existing solve, the copy out; `save`: 3 x 2n doubles.  Whatever this returns, the caller puts the contents back
static int solve_rhs_run(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* b, double* x, double* save, pph_solve_info* info,
                         double* hist, int hist_cap) {
  const int64_t n = ctx->n, N = 2 * n;
  const int grid = (int)(ceil_div64(N, 256) < 2048 ? ceil_div64(N, 256) : 2048);
  la_copy(ctx, save, ctx->rhs.p, N);
  la_copy(ctx, save + N, ctx->u0.p, N);
  la_copy(ctx, save + 2 * N, ctx->sol.p, N);
  hipLaunchKernelGGL(k_mask_free, dim3(grid), dim3(256), 0, ctx->stream, ctx->rhs.p, b, ctx->bcmask[0].p, ctx->bcmask[1].p, n);
  la_set(ctx, ctx->u0.p, 0.0, N);
  PPH_HIP(ctx, hipGetLastError());
  // a right-hand side without an entry on a free dof: x = 0 without entering a Krylov loop (no 0 / 0 in the relative tests);
  // the norm is the one pph_solve_device takes first
  la_dot(ctx, ctx->rhs.p, ctx->rhs.p, N, 0);
  PPH_TRY(la_fetch(ctx, 0, 1));
  if (ctx->h_scal[0] == 0.0) {
    la_set(ctx, x, 0.0, N);
    PPH_HIP(ctx, hipGetLastError());
    if (info) {
      info->iterations = 0; info->inner_iterations = 0; info->converged = 1; info->inner_failed = 0;
      info->resnorm = 0.0; info->rhs_norm = 0.0;
    }
    if (hist && hist_cap > 0) hist[0] = 0.0;
    return PPH_OK;
  }
  const int st = pph_solve_device(ctx, cfg, info, hist, hist_cap);
  if (st < 0 && st != PPH_ERR_DIVERGED) return st;
  // u0 = 0, so the solution is the correction; the constrained dofs hold exactly 0
  hipLaunchKernelGGL(k_mask_free, dim3(grid), dim3(256), 0, ctx->stream, x, ctx->sol.p, ctx->bcmask[0].p, ctx->bcmask[1].p, n);
  PPH_HIP(ctx, hipGetLastError());
  return st;
}

extern "C" int pph_solve_rhs_device(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* b_dev, double* x_dev,
                                    pph_solve_info* info, double* hist, int hist_cap) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, ctx->asm_ok, "pph_solve_rhs before pph_assemble_dpp");
  PPH_REQUIRE(ctx, ctx->world == 1, "pph_solve_rhs is implemented for single-context meshes");
  PPH_REQUIRE(ctx, b_dev != nullptr && x_dev != nullptr, "pph_solve_rhs: NULL buffer");
  PPH_REQUIRE(ctx, b_dev != x_dev, "pph_solve_rhs: b and x must be different buffers");
  PPH_TRY(validate_cfg(ctx, cfg));
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t N = 2 * ctx->n;
  DevBuf<double> save;
  PPH_TRY(save.alloc(ctx, (size_t)(3 * N)));
  int st = solve_rhs_run(ctx, cfg, b_dev, x_dev, save.p, info, hist, hist_cap);
  const std::string msg = ctx->err;   // (the solve's message survives the clean-up)
  // the context's right-hand side, lifting and solution again hold the bits they held before the call
  la_copy(ctx, ctx->rhs.p, save.p, N);
  la_copy(ctx, ctx->u0.p, save.p + N, N);
  la_copy(ctx, ctx->sol.p, save.p + 2 * N, N);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (save is freed below; the caller's arrays are free again)
  save.release();
  if (e != hipSuccess && st >= 0) {
    pph_set_error(ctx, "pph_solve_rhs: restoring the context's vectors failed: %s", hipGetErrorString(e));
    return PPH_ERR_HIP;
  }
  if (st < 0) ctx->err = msg;
  return st;
}

extern "C" int pph_solve_rhs(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* b_host, double* x_host, pph_solve_info* info,
                             double* hist, int hist_cap) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, ctx->asm_ok, "pph_solve_rhs before pph_assemble_dpp");
  PPH_REQUIRE(ctx, ctx->world == 1, "pph_solve_rhs is implemented for single-context meshes");
  PPH_REQUIRE(ctx, b_host != nullptr && x_host != nullptr, "pph_solve_rhs: NULL buffer");
  PPH_REQUIRE(ctx, b_host != x_host, "pph_solve_rhs: b and x must be different buffers");
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = 2 * (size_t)ctx->n;
  DevBuf<double> bx;
  PPH_TRY(bx.alloc(ctx, 2 * N));
  int st = PPH_OK;
  hipError_t e = hipMemcpyAsync(bx.p, b_host, sizeof(double) * N, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    st = pph_solve_rhs_device(ctx, cfg, bx.p, bx.p + N, info, hist, hist_cap);
    if (st >= 0 || st == PPH_ERR_DIVERGED) {
      e = hipMemcpyAsync(x_host, bx.p + N, sizeof(double) * N, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
  }
  bx.release();
  if (e != hipSuccess) {
    pph_set_error(ctx, "pph_solve_rhs: copy failed: %s", hipGetErrorString(e));
    return PPH_ERR_HIP;
  }
  return st;
}
