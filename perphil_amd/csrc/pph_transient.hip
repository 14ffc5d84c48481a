// Transient DPP: the right-hand side of a theta step in delta form, the shifted assembly's share of the lifting, and the
// step loop (second half of this file).
//
// No reference counterpart: the reference solves the steady state of dpp_form (src/perphil/forms/dpp.py:95-132) only.  With a
// storage coefficient S_f > 0 per network,
//   S1 dp1/dt - div(k1/mu grad p1) + beta/mu (p1 - p2) = 0,   S2 dp2/dt - div(k2/mu grad p2) - beta/mu (p1 - p2) = 0,
// a theta step in delta form solves (Sigma M / dt + theta A) d = -F A_unel p^n, p^{n+1} = p^n + d, with A_unel the un-eliminated
// operator of pph_dpp_nodal_flux and F the projection that zeroes the constrained dofs.  This unit forms that right-hand side,
//   b1 = -F1 ((k1/mu) K p1 + (beta/mu) M (p1 - p2)),   b2 = -F2 ((k2/mu) K p2 - (beta/mu) M (p1 - p2)),
// for both fields in one pass.
//
//   k_step_rhs      degree-1 boxes (node i at i / n, pph_mesh.hip): matrix-free.  One work item per node; neither K nor M nor the
//                   dof map is read.  The row of a node is the sum over its incident boxes of the rows of the BOX matrices
//                   KB[a][b], MB[a][b] (a, b box corners x + 2y + 4z), closed forms of the canonical cell formed on the host:
//                     Q1: KB = |box| sum_d n_d^2 (S along d, Mm along the others), MB = |box| Mm x Mm (x Mm),
//                         S = [1 -1; -1 1], Mm = [2 1; 1 2] / 6 (the forms of k_dpp_bilinear, pph_adjoint.hip);
//                     P1: the sum over the box's sub-cells (p2_simplex_vertex) of K_e[r][s] = |c| sum_d n_d^2 e_d[r] e_d[s]
//                         (e_d = +1 / -1 at the upper / lower end of the sub-cell's edge along axis d, else 0) and
//                         M_e[r][s] = |c| (1 + delta_rs) / ((D + 1)(D + 2)).
//                   On tensor cells the sum over the boxes factorises: per direction the assembled 1-D rows
//                   s = (-lo, lo + hi, -hi), m = (lo, 2 (lo + hi), hi) / 6 (lo / hi = 1 where the box below / above exists) and
//                   K_row(o) = |box| sum_d n_d^2 s_d(o_d) prod_{e != d} m_e(o_e), M_row(o) = |box| prod_e m_e(o_e): no table.
//                   A box outside the mesh is skipped by index arithmetic: the node at position i along e is corner 1 of the
//                   box below (exists when i > 0) and corner 0 of the box above (exists when i < n_e).  Per stencil offset the
//                   coefficients of the existing boxes are summed first (registers; the offsets outside the cell kind's stencil
//                   are dropped at compile time), then p1 and p2 of that neighbour are loaded once: 9 / 7 / 27 / 15 pairs of
//                   loads per node, all but the node's own served by the caches (consecutive lanes are consecutive nodes
//                   along x).  HBM traffic per node: 16 B of p, 2 B of masks, 16 B of b.
//   fallback        degree 2, or option "asm_uniform" 0 (the stored-coordinate path of the assembly): the CSR walk of
//                   pph_dpp_nodal_flux on the stored K and M, then k_step_mask (mask and sign in place).
//
// Determinism: a node's sums run in a fixed order, no atomics; two calls give the same bits.
#include "pph_internal.h"
#include "pph_p2.h"

#define STEP_MAX_BLOCKS 2048   // grid cap of k_step_rhs (256 nodes per workgroup and pass)

struct StepTab { double K[64], M[64]; };   // box matrices [a * NC + b], NC = 2^dim corners (simplices)
struct StepGeo { double cd[3], vol; };     // n_d^2 |box| and |box| (tensor cells)

template <int KIND>
struct StepCell {
  static constexpr int DIM = (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_TRI) ? 2 : 3;
  static constexpr int NC = 1 << DIM;
  static constexpr bool TENSOR = (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_HEX);
  // offset (ox, oy, oz) in {-1, 0, 1}^3 belongs to the stencil of the cell kind (make_stencil)
  __host__ __device__ static constexpr bool in_stencil(int ox, int oy, int oz) {
    if (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_HEX) return true;
    if (KIND == PPH_CELL_TRI) return !(ox == oy && ox != 0);   // x, y and the "left" diagonal (-1, +1)
    return (ox >= 0 && oy >= 0 && oz >= 0) || (ox <= 0 && oy <= 0 && oz <= 0);   // Kuhn edges
  }
};

// LIFT: the same gather with the mass rows alone, out[f] -= c_f F_f M q_f (ca, cc = sigma1, sigma2; q1, q2 the Dirichlet values):
// the shifted assembly's share of the lifted right-hand side (pph_step_lift)
template <int KIND, bool LIFT>
__global__ __launch_bounds__(256) void k_step_rhs(const double* __restrict__ q1, const double* __restrict__ q2,
                                                  const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int px, int py,
                                                  int pz, int64_t n, double ca, double cb, double cc, StepGeo g, StepTab tab,
                                                  double* __restrict__ out) {
  using C = StepCell<KIND>;
  constexpr int DIM = C::DIM, NC = C::NC;
  const int64_t pxy = (int64_t)px * py;
  for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
    // (32-bit index arithmetic where the mesh allows: a 64-bit division is a long instruction sequence on this hardware)
    int i, j, k;
    if (n < ((int64_t)1 << 31)) {
      const uint32_t r32 = (uint32_t)row, t32 = r32 / (uint32_t)px;
      i = (int)(r32 - t32 * (uint32_t)px);
      k = (DIM == 3) ? (int)(t32 / (uint32_t)py) : 0;
      j = (int)(t32 - (uint32_t)k * (uint32_t)py);
    } else {
      i = (int)(row % px); j = (int)((row / px) % py); k = (DIM == 3) ? (int)(row / pxy) : 0;
    }
    // ex[e][a_e]: the box of which the node is corner a_e along direction e exists (a_e = 0: the box above, 1: the box below)
    const bool ex[3][2] = {{i < px - 1, i > 0}, {j < py - 1, j > 0}, {DIM == 3 ? k < pz - 1 : true, DIM == 3 ? k > 0 : false}};
    // tensor cells: per direction the assembled rows of the 1-D stiffness and mass matrices at offsets -1, 0, +1
    double s1d[3][3], m1d[3][3];
    if constexpr (C::TENSOR) {
#pragma unroll
      for (int e = 0; e < DIM; ++e) {
        const double lo = ex[e][1] ? 1.0 : 0.0, hi = ex[e][0] ? 1.0 : 0.0;
        s1d[e][0] = -lo; s1d[e][1] = lo + hi; s1d[e][2] = -hi;
        m1d[e][0] = lo * (1.0 / 6.0); m1d[e][1] = (lo + hi) * (1.0 / 3.0); m1d[e][2] = hi * (1.0 / 6.0);
      }
    }
    double s1 = 0.0, s2 = 0.0, sm = 0.0;
#pragma unroll
    for (int oz = (DIM == 3 ? -1 : 0); oz <= (DIM == 3 ? 1 : 0); ++oz)
#pragma unroll
      for (int oy = -1; oy <= 1; ++oy)
#pragma unroll
        for (int ox = -1; ox <= 1; ++ox) {
          if (!C::in_stencil(ox, oy, oz)) continue;
          double wk = 0.0, wm = 0.0;
          bool any = false;
          if constexpr (C::TENSOR) {
            // the neighbour exists when a box exists on its side in every direction it is offset in
            any = (ox == 0 || ex[0][ox > 0 ? 0 : 1]) && (oy == 0 || ex[1][oy > 0 ? 0 : 1]) &&
                  (DIM == 2 || oz == 0 || ex[2][oz > 0 ? 0 : 1]);
            const double sx = s1d[0][ox + 1], sy = s1d[1][oy + 1], mx = m1d[0][ox + 1], my = m1d[1][oy + 1];
            if constexpr (DIM == 2) {
              wk = g.cd[0] * (sx * my) + g.cd[1] * (mx * sy);
              wm = g.vol * (mx * my);
            } else {
              const double sz = s1d[2][oz + 1], mz = m1d[2][oz + 1], mxy = mx * my;
              wk = (g.cd[0] * (sx * my) + g.cd[1] * (mx * sy)) * mz + g.cd[2] * (mxy * sz);
              wm = g.vol * (mxy * mz);
            }
          } else {
#pragma unroll
            for (int a = 0; a < NC; ++a) {
              const int ax = a & 1, ay = (a >> 1) & 1, az = (a >> 2) & 1;
              const int bx = ax + ox, by = ay + oy, bz = az + oz;
              if (bx < 0 || bx > 1 || by < 0 || by > 1 || bz < 0 || bz > 1) continue;   // (the neighbour is no corner of that box)
              const int b = bx + 2 * by + 4 * bz;
              const bool e = ex[0][ax] && ex[1][ay] && (DIM == 3 ? ex[2][az] : true);
              // (the box matrices are symmetric: one entry per corner pair travels as a kernel argument)
              const int t = (a < b ? a : b) * NC + (a < b ? b : a);
              wk += e ? tab.K[t] : 0.0;
              wm += e ? tab.M[t] : 0.0;
              any = any || e;
            }
          }
          if (any) {   // (a box holds both nodes: the neighbour is inside the mesh)
            const int64_t nb = row + ox + (int64_t)px * oy + pxy * oz;
            const double p1 = q1[nb], p2 = q2[nb];
            if constexpr (LIFT) {
              s1 += wm * p1;
              s2 += wm * p2;
            } else {
              s1 += wk * p1;
              s2 += wk * p2;
              sm += wm * (p1 - p2);
            }
          }
        }
    if constexpr (LIFT) {
      if (!m0[row]) out[row] -= ca * s1;
      if (!m1[row]) out[n + row] -= cc * s2;
    } else {
      const double r1 = ca * s1 + cb * sm, r2 = cc * s2 - cb * sm;
      out[row] = m0[row] ? 0.0 : -r1;
      out[n + row] = m1[row] ? 0.0 : -r2;
    }
  }
}

// b = (mask != 0) ? 0 : -b over both fields, in place (the CSR fallback)
__global__ __launch_bounds__(256) void k_step_mask(double* __restrict__ b, const uint8_t* __restrict__ m0,
                                                   const uint8_t* __restrict__ m1, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 2 * n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t m = (i < n) ? m0[i] : m1[i - n];
    b[i] = m ? 0.0 : -b[i];
  }
}

// the box matrices of the canonical cell of an nd[0] x nd[1] (x nd[2]) box mesh
static void step_box_tables(int kind, const int* nd, StepTab* tab) {
  const int dim = (kind == PPH_CELL_QUAD || kind == PPH_CELL_TRI) ? 2 : 3, nc = 1 << dim;
  for (int q = 0; q < 64; ++q) tab->K[q] = tab->M[q] = 0.0;
  double vol = 1.0;
  for (int d = 0; d < dim; ++d) vol /= (double)nd[d];
  if (kind == PPH_CELL_QUAD || kind == PPH_CELL_HEX) {
    auto s1 = [](int i, int j) { return i == j ? 1.0 : -1.0; };
    auto m1 = [](int i, int j) { return i == j ? 1.0 / 3.0 : 1.0 / 6.0; };
    for (int a = 0; a < nc; ++a)
      for (int b = 0; b < nc; ++b) {
        double kk = 0.0, mm = 1.0;
        for (int d = 0; d < dim; ++d) {
          double t = (double)nd[d] * (double)nd[d];
          for (int e = 0; e < dim; ++e) t *= (e == d) ? s1((a >> e) & 1, (b >> e) & 1) : m1((a >> e) & 1, (b >> e) & 1);
          kk += t;
          mm *= m1((a >> d) & 1, (b >> d) & 1);
        }
        tab->K[a * nc + b] = vol * kk;
        tab->M[a * nc + b] = vol * mm;
      }
    return;
  }
  const int cpb = p2_cells_per_box(kind);
  const double vc = vol / (double)cpb;
  for (int sub = 0; sub < cpb; ++sub) {
    int v[4];
    for (int r = 0; r <= dim; ++r) v[r] = p2_simplex_vertex(kind, sub, r);
    for (int r = 0; r <= dim; ++r)
      for (int s = 0; s <= dim; ++s) {
        double kk = 0.0;
        for (int d = 0; d < dim; ++d) {
          // the sub-cell's edge along axis d: the pair of its vertices that differ in bit d alone
          int lo = -1, up = -1;
          for (int q = 0; q <= dim; ++q)
            for (int t = 0; t <= dim; ++t)
              if (v[t] == (v[q] | (1 << d)) && v[t] != v[q]) { lo = q; up = t; }
          const double er = (r == up) ? 1.0 : (r == lo ? -1.0 : 0.0), es = (s == up) ? 1.0 : (s == lo ? -1.0 : 0.0);
          kk += (double)nd[d] * (double)nd[d] * er * es;
        }
        tab->K[v[r] * nc + v[s]] += vc * kk;
        tab->M[v[r] * nc + v[s]] += vc * (r == s ? 2.0 : 1.0) / (double)((dim + 1) * (dim + 2));
      }
  }
}

template <int KIND>
static void step_launch(pph_ctx* ctx, bool lift, int grid, const double* q1, const double* q2, double a, double b, double c,
                        const StepGeo& g, const StepTab& tab, double* out) {
  const MeshData& m = ctx->mesh;
  if (lift)
    hipLaunchKernelGGL((k_step_rhs<KIND, true>), dim3(grid), dim3(256), 0, ctx->stream, q1, q2, ctx->bcmask[0].p, ctx->bcmask[1].p,
                       m.px, m.py, m.pzl, m.n, a, b, c, g, tab, out);
  else
    hipLaunchKernelGGL((k_step_rhs<KIND, false>), dim3(grid), dim3(256), 0, ctx->stream, q1, q2, ctx->bcmask[0].p, ctx->bcmask[1].p,
                       m.px, m.py, m.pzl, m.n, a, b, c, g, tab, out);
}

// the matrix-free launch: b = -F A_unel (q1, q2), or with lift out[f] -= c_f F_f M q_f (a = sigma1, c = sigma2)
static int step_matfree_launch(pph_ctx* ctx, bool lift, const double* q1, const double* q2, double a, double bb, double c,
                               double* out) {
  const MeshData& m = ctx->mesh;
  const int nd[3] = {m.nx, m.ny, (m.dim == 3) ? m.nzl : 1};
  StepTab tab;
  step_box_tables(m.kind, nd, &tab);
  StepGeo g;
  g.vol = 1.0;
  for (int d = 0; d < m.dim; ++d) g.vol /= (double)nd[d];
  for (int d = 0; d < 3; ++d) g.cd[d] = (d < m.dim) ? (double)nd[d] * (double)nd[d] * g.vol : 0.0;
  const int64_t nb = ceil_div64(m.n, 256);
  const int grid = (int)(nb < 1 ? 1 : (nb < STEP_MAX_BLOCKS ? nb : STEP_MAX_BLOCKS));
  if (m.kind == PPH_CELL_QUAD) step_launch<PPH_CELL_QUAD>(ctx, lift, grid, q1, q2, a, bb, c, g, tab, out);
  else if (m.kind == PPH_CELL_TRI) step_launch<PPH_CELL_TRI>(ctx, lift, grid, q1, q2, a, bb, c, g, tab, out);
  else if (m.kind == PPH_CELL_HEX) step_launch<PPH_CELL_HEX>(ctx, lift, grid, q1, q2, a, bb, c, g, tab, out);
  else step_launch<PPH_CELL_TET>(ctx, lift, grid, q1, q2, a, bb, c, g, tab, out);
  PPH_HIP(ctx, hipGetLastError());
  return PPH_OK;
}

int pph_step_lift(pph_ctx* ctx, double sigma1, double sigma2, const double* g1, const double* g2, double* rhs) {
  PPH_REQUIRE(ctx, ctx->mesh.degree == 1 && ctx->world == 1, "shifted lifting: degree-1 single-context meshes");
  return step_matfree_launch(ctx, true, g1, g2, sigma1, 0.0, sigma2, rhs);
}

// whether the step right-hand side of this context runs matrix-free
static bool step_matfree(const pph_ctx* ctx) {
  const MeshData& m = ctx->mesh;
  if (m.degree != 1 || !ctx->asm_uniform) return false;
  // (multilinear cells: every edge was checked against the canonical one at mesh build; simplices are built on the same lattice)
  return (m.kind == PPH_CELL_TRI || m.kind == PPH_CELL_TET) ? true : m.uniform;
}

// b = -F A_unel p, enqueued on the context stream
static int step_rhs_dev(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p, double* b) {
  const MeshData& m = ctx->mesh;
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  if (!step_matfree(ctx)) {
    PPH_TRY(pph_nodal_flux_launch(ctx, k1, k2, beta, mu, p, b));
    const int64_t nb = ceil_div64(2 * m.n, 256);
    hipLaunchKernelGGL(k_step_mask, dim3((int)(nb < STEP_MAX_BLOCKS ? nb : STEP_MAX_BLOCKS)), dim3(256), 0, ctx->stream, b,
                       ctx->bcmask[0].p, ctx->bcmask[1].p, m.n);
    PPH_HIP(ctx, hipGetLastError());
    return PPH_OK;
  }
  return step_matfree_launch(ctx, false, p, p + m.n, k1 / mu, beta / mu, k2 / mu, b);
}

// (for the backward loop of pph_transient_adjoint.hip)
int pph_step_rhs_launch(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p, double* b) {
  return step_rhs_dev(ctx, k1, k2, beta, mu, p, b);
}

static int step_check(pph_ctx* ctx, const char* who, double mu, const double* p, const double* b) {
  PPH_REQUIRE(ctx, ctx->mesh_ok, "%s before pph_mesh_build", who);
  PPH_REQUIRE(ctx, ctx->world == 1, "%s is implemented for single-context meshes", who);
  PPH_REQUIRE(ctx, p != nullptr && b != nullptr, "%s: NULL buffer", who);
  PPH_REQUIRE(ctx, p != b, "%s: p and b must be different buffers", who);
  PPH_REQUIRE(ctx, mu != 0.0, "%s: mu must not be 0", who);
  return PPH_OK;
}

extern "C" int pph_dpp_step_rhs_device(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p_dev,
                                       double* b_dev) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(step_check(ctx, "pph_dpp_step_rhs_device", mu, p_dev, b_dev));
  PPH_TRY(step_rhs_dev(ctx, k1, k2, beta, mu, p_dev, b_dev));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the caller's arrays are free again when the call returns)
  return PPH_OK;
}

extern "C" int pph_dpp_step_rhs(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p_host, double* b_host) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(step_check(ctx, "pph_dpp_step_rhs", mu, p_host, b_host));
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = 2 * (size_t)ctx->mesh.n;
  DevBuf<double> pb;   // p, then b
  PPH_TRY(pb.alloc(ctx, 2 * N));
  int st = PPH_OK;
  hipError_t e = hipMemcpyAsync(pb.p, p_host, sizeof(double) * N, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    st = step_rhs_dev(ctx, k1, k2, beta, mu, pb.p, pb.p + N);
    if (st == PPH_OK) e = hipMemcpyAsync(b_host, pb.p + N, sizeof(double) * N, hipMemcpyDeviceToHost, ctx->stream);
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  pb.release();
  if (st < 0) return st;
  if (e != hipSuccess) {
    pph_set_error(ctx, "pph_dpp_step_rhs: copy failed: %s", hipGetErrorString(e));
    return PPH_ERR_HIP;
  }
  return PPH_OK;
}

// ---- the step loop ---------------------------------------------------------------------------------------------------
// pph_transient_begin assembles the step operator Sigma M / dt + theta A through pph_assemble_dpp_shifted with
// (theta k1, theta k2, theta beta, mu, S1 / dt, S2 / dt) and records the steady coefficients.  pph_transient_steps* then runs
//   b = -F A_unel p (k_step_rhs, straight into the context's right-hand side);  (Sigma M / dt + theta A) d = b;  p += d
// with the solve loop of pph_solve_device on whatever path cfg names.  As pph_solve_rhs does per solve, the CONTENTS of the
// context's right-hand side, lifting and solution are exchanged with saved copies - once per call - and put back on return.
// Per step the host reads one pair of scalars: ||b_s||^2 and, with it, ||d_{s-1}||^2 that k_step_update left behind.
// pph_transient_steps_sources*: between the right-hand side and its norm, b_s += F sum_k coef[s][k] L_k with the context's
// source set (pph_sources.hip); the coefficient rows travel once per call, behind the saved vectors in the call's allocation.

// p = Dirichlet value on the constrained dofs of either field
__global__ __launch_bounds__(256) void k_step_constrain(double* __restrict__ p, const uint8_t* __restrict__ m0,
                                                        const uint8_t* __restrict__ m1, const double* __restrict__ g0,
                                                        const double* __restrict__ g1, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 2 * n; i += (int64_t)gridDim.x * blockDim.x) {
    const bool second = i >= n;
    const int64_t j = second ? i - n : i;
    if ((second ? m1[j] : m0[j]) & 1) p[i] = second ? g1[j] : g0[j];
  }
}

// p += d on the free dofs (d is 0 on the others) and part[block] = this workgroup's share of ||d||^2, fixed order
__global__ __launch_bounds__(256) void k_step_update(double* __restrict__ p, const double* __restrict__ d,
                                                     const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int64_t n,
                                                     double* __restrict__ part) {
  __shared__ double lds[256];
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 2 * n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t m = (i < n) ? m0[i] : m1[i - n];
    const double di = m ? 0.0 : d[i];
    p[i] += di;
    acc += di * di;
  }
  lds[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = lds[0];
}

// out[0] = sum of part[i], i < nblocks, one workgroup, fixed order
__global__ __launch_bounds__(256) void k_step_sum(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  __shared__ double lds[256];
  double v = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) v += part[i];
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = lds[0];
}

extern "C" int pph_transient_begin(pph_ctx* ctx, double k1, double k2, double beta, double mu, double S1, double S2, double theta,
                                   double dt, int monolithic) {
  if (!ctx) return PPH_ERR_INVALID;
  ctx->tr_on = false;
  PPH_REQUIRE(ctx, ctx->mesh_ok, "pph_transient_begin before pph_mesh_build");
  PPH_REQUIRE(ctx, ctx->world == 1, "pph_transient_begin is implemented for single-context meshes");
  PPH_REQUIRE(ctx, S1 > 0 && S2 > 0 && S1 < INFINITY && S2 < INFINITY, "pph_transient_begin: storage coefficients must be finite and > 0, got %g, %g", S1, S2);
  PPH_REQUIRE(ctx, dt > 0 && dt < INFINITY, "pph_transient_begin: dt must be finite and > 0, got %g", dt);
  PPH_REQUIRE(ctx, theta >= 0.5 && theta <= 1.0, "pph_transient_begin: theta must lie in [1/2, 1], got %g", theta);
  PPH_TRY(pph_assemble_dpp_shifted(ctx, theta * k1, theta * k2, theta * beta, mu, S1 / dt, S2 / dt, monolithic));
  ctx->tr_coef[0] = k1; ctx->tr_coef[1] = k2; ctx->tr_coef[2] = beta; ctx->tr_coef[3] = mu;
  ctx->tr_theta = theta;
  ctx->tr_asm_epoch = ctx->asm_epoch;
  ctx->tr_bc_epoch = ctx->bc_epoch;
  ctx->tr_b0 = -1.0;
  ctx->tr_on = true;
  return PPH_OK;
}

// the loop between the exchange and the restore; `save`: 3 x 2n doubles, then STEP_MAX_BLOCKS partial sums; `traj`: NULL, or
// [nsteps + 1][2n] on the device: row 0 receives p after k_step_constrain, row s + 1 after the update of step s; `coef`: NULL, or
// the coefficient rows [nsteps][K] of the context's source set on the device: b_s += F sum_k coef[s][k] L_k (pph_sources.hip)
static int transient_run(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p, int nsteps, double steady_tol, pph_solve_info* infos,
                         double* norms, int* steps_done, double* save, double* traj, const double* coef, int64_t K) {
  const int64_t n = ctx->n, N = 2 * n;
  const int grid = (int)(ceil_div64(N, 256) < STEP_MAX_BLOCKS ? ceil_div64(N, 256) : STEP_MAX_BLOCKS);
  double* part = save + 3 * N;
  la_copy(ctx, save, ctx->rhs.p, N);
  la_copy(ctx, save + N, ctx->u0.p, N);
  la_copy(ctx, save + 2 * N, ctx->sol.p, N);
  hipLaunchKernelGGL(k_step_constrain, dim3(grid), dim3(256), 0, ctx->stream, p, ctx->bcmask[0].p, ctx->bcmask[1].p, ctx->g[0].p,
                     ctx->g[1].p, n);
  la_set(ctx, ctx->u0.p, 0.0, N);
  la_set(ctx, ctx->scal.p + 1, 0.0, 1);
  if (traj) la_copy(ctx, traj, p, N);
  PPH_HIP(ctx, hipGetLastError());
  int s = 0;
  for (; s < nsteps; ++s) {
    PPH_TRY(step_rhs_dev(ctx, ctx->tr_coef[0], ctx->tr_coef[1], ctx->tr_coef[2], ctx->tr_coef[3], p, ctx->rhs.p));
    if (coef) PPH_TRY(src_apply_launch(ctx, coef + (int64_t)s * K, ctx->rhs.p));
    la_dot(ctx, ctx->rhs.p, ctx->rhs.p, N, 0);
    PPH_TRY(la_fetch(ctx, 0, 2));   // ||b_s||^2 and the ||d_{s-1}||^2 the last update left in slot 1
    const double bn = sqrt(ctx->h_scal[0]);
    if (s > 0 && norms) norms[2 * (s - 1) + 1] = sqrt(ctx->h_scal[1]);
    if (ctx->tr_b0 < 0.0) ctx->tr_b0 = bn;   // (b_0 of the run: the first right-hand side after pph_transient_begin)
    if (steady_tol > 0.0 && bn <= steady_tol * ctx->tr_b0) break;
    pph_solve_info info;
    info.iterations = 0; info.inner_iterations = 0; info.converged = 1; info.inner_failed = 0; info.resnorm = 0.0; info.rhs_norm = 0.0;
    int st = PPH_OK;
    if (bn != 0.0) {   // (a right-hand side without an entry on a free dof: d = 0 without entering a Krylov loop)
      st = pph_solve_device(ctx, cfg, &info, nullptr, 0);
      if (st < 0 && st != PPH_ERR_DIVERGED) return st;
    } else {
      la_set(ctx, ctx->sol.p, 0.0, N);
    }
    if (infos) infos[s] = info;
    if (norms) { norms[2 * s] = bn; norms[2 * s + 1] = 0.0; }
    if (st == PPH_ERR_DIVERGED) { *steps_done = s; return st; }   // (p holds the last completed step)
    hipLaunchKernelGGL(k_step_update, dim3(grid), dim3(256), 0, ctx->stream, p, ctx->sol.p, ctx->bcmask[0].p, ctx->bcmask[1].p, n, part);
    hipLaunchKernelGGL(k_step_sum, dim3(1), dim3(256), 0, ctx->stream, part, grid, ctx->scal.p + 1);
    if (traj) la_copy(ctx, traj + (int64_t)(s + 1) * N, p, N);
    PPH_HIP(ctx, hipGetLastError());
  }
  *steps_done = s;
  if (s > 0 && norms) {
    PPH_TRY(la_fetch(ctx, 1, 1));
    norms[2 * (s - 1) + 1] = sqrt(ctx->h_scal[1]);
  }
  return PPH_OK;
}

// `sources`: the call is one of pph_transient_steps_sources*: coef_host [nsteps][K] is uploaded once, behind the saved vectors
static int transient_steps_dev(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_dev, int nsteps, double steady_tol,
                               pph_solve_info* infos, double* norms, int* steps_done, double* traj, bool sources = false,
                               const double* coef_host = nullptr, int64_t K = 0) {
  if (steps_done) *steps_done = 0;
  PPH_REQUIRE(ctx, ctx->world == 1, "pph_transient_steps is implemented for single-context meshes");
  PPH_REQUIRE(ctx, ctx->tr_on, "pph_transient_steps before pph_transient_begin");
  PPH_REQUIRE(ctx, ctx->asm_ok && ctx->asm_epoch == ctx->tr_asm_epoch,
              "pph_transient_steps: the system was assembled again (or dropped) after pph_transient_begin");
  PPH_REQUIRE(ctx, ctx->bc_epoch == ctx->tr_bc_epoch, "pph_transient_steps: the Dirichlet sets changed after pph_transient_begin");
  PPH_REQUIRE(ctx, p_dev != nullptr && steps_done != nullptr && cfg != nullptr, "pph_transient_steps: NULL buffer");
  PPH_REQUIRE(ctx, nsteps >= 1, "pph_transient_steps: nsteps must be >= 1, got %d", nsteps);
  if (sources) {
    PPH_REQUIRE(ctx, ctx->src.on, "pph_transient_steps_sources: the context holds no source set (pph_sources_set)");
    PPH_REQUIRE(ctx, ctx->src.count() == K, "pph_transient_steps_sources: coef has %lld columns, the context's source set %lld sources",
                (long long)K, (long long)ctx->src.count());
    PPH_REQUIRE(ctx, K == 0 || coef_host != nullptr, "pph_transient_steps_sources: NULL buffer");
  }
  PPH_TRY(validate_cfg(ctx, cfg));
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t N = 2 * ctx->n;
  const size_t ncoef = sources ? (size_t)nsteps * (size_t)K : 0;
  DevBuf<double> save;   // the saved vectors, the partial sums, then the coefficient rows: the call's one allocation
  PPH_TRY(save.alloc(ctx, (size_t)(3 * N + STEP_MAX_BLOCKS) + ncoef));
  double* coef = sources ? save.p + (size_t)(3 * N + STEP_MAX_BLOCKS) : nullptr;
  if (ncoef) {
    const hipError_t ec = hipMemcpyAsync(coef, coef_host, sizeof(double) * ncoef, hipMemcpyHostToDevice, ctx->stream);
    if (ec != hipSuccess) {
      (void)hipStreamSynchronize(ctx->stream);
      save.release();
      pph_set_error(ctx, "pph_transient_steps_sources: uploading coef failed: %s", hipGetErrorString(ec));
      return PPH_ERR_HIP;
    }
  }
  int st = transient_run(ctx, cfg, p_dev, nsteps, steady_tol, infos, norms, steps_done, save.p, traj, coef, K);
  const std::string msg = ctx->err;   // (the solve's message survives the clean-up)
  // the context's right-hand side, lifting and solution again hold the bits they held before the call
  la_copy(ctx, ctx->rhs.p, save.p, N);
  la_copy(ctx, ctx->u0.p, save.p + N, N);
  la_copy(ctx, ctx->sol.p, save.p + 2 * N, N);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (save is freed below; the caller's array is free again)
  save.release();
  if (e != hipSuccess && st >= 0) {
    pph_set_error(ctx, "pph_transient_steps: restoring the context's vectors failed: %s", hipGetErrorString(e));
    return PPH_ERR_HIP;
  }
  if (st < 0) ctx->err = msg;
  return st;
}

extern "C" int pph_transient_steps_device(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_dev, int nsteps, double steady_tol,
                                          pph_solve_info* infos, double* norms, int* steps_done) {
  if (!ctx) return PPH_ERR_INVALID;
  return transient_steps_dev(ctx, cfg, p_dev, nsteps, steady_tol, infos, norms, steps_done, nullptr);
}

extern "C" int pph_transient_steps_record_device(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_dev, int nsteps,
                                                 double steady_tol, pph_solve_info* infos, double* norms, int* steps_done,
                                                 double* traj_dev) {
  if (!ctx) return PPH_ERR_INVALID;
  if (steps_done) *steps_done = 0;
  PPH_REQUIRE(ctx, traj_dev != nullptr, "pph_transient_steps_record: NULL buffer");
  return transient_steps_dev(ctx, cfg, p_dev, nsteps, steady_tol, infos, norms, steps_done, traj_dev);
}

// the host variants: p (and the trajectory) live on the device for the call
static int transient_steps_host(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_host, int nsteps, double steady_tol,
                                pph_solve_info* infos, double* norms, int* steps_done, double* traj_host, bool record,
                                bool sources = false, const double* coef_host = nullptr, int64_t K = 0) {
  if (steps_done) *steps_done = 0;
  PPH_REQUIRE(ctx, ctx->world == 1, "pph_transient_steps is implemented for single-context meshes");
  PPH_REQUIRE(ctx, ctx->tr_on, "pph_transient_steps before pph_transient_begin");
  PPH_REQUIRE(ctx, p_host != nullptr && steps_done != nullptr && cfg != nullptr && (!record || traj_host != nullptr),
              "pph_transient_steps: NULL buffer");
  PPH_REQUIRE(ctx, nsteps >= 1, "pph_transient_steps: nsteps must be >= 1, got %d", nsteps);
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = 2 * (size_t)ctx->n;
  DevBuf<double> p;   // p, then the trajectory
  PPH_TRY(p.alloc(ctx, record ? N * ((size_t)nsteps + 2) : N));
  double* traj = record ? p.p + N : nullptr;
  int st = PPH_OK;
  hipError_t e = hipMemcpyAsync(p.p, p_host, sizeof(double) * N, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    st = transient_steps_dev(ctx, cfg, p.p, nsteps, steady_tol, infos, norms, steps_done, traj, sources, coef_host, K);
    if (st >= 0 || st == PPH_ERR_DIVERGED) {
      e = hipMemcpyAsync(p_host, p.p, sizeof(double) * N, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess && record)
        e = hipMemcpyAsync(traj_host, traj, sizeof(double) * N * ((size_t)*steps_done + 1), hipMemcpyDeviceToHost, ctx->stream);
    }
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  p.release();
  if (e != hipSuccess && st >= 0) {
    pph_set_error(ctx, "pph_transient_steps: copy failed: %s", hipGetErrorString(e));
    return PPH_ERR_HIP;
  }
  return st;
}

extern "C" int pph_transient_steps(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_host, int nsteps, double steady_tol,
                                   pph_solve_info* infos, double* norms, int* steps_done) {
  if (!ctx) return PPH_ERR_INVALID;
  return transient_steps_host(ctx, cfg, p_host, nsteps, steady_tol, infos, norms, steps_done, nullptr, false);
}

extern "C" int pph_transient_steps_record(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_host, int nsteps, double steady_tol,
                                          pph_solve_info* infos, double* norms, int* steps_done, double* traj_host) {
  if (!ctx) return PPH_ERR_INVALID;
  return transient_steps_host(ctx, cfg, p_host, nsteps, steady_tol, infos, norms, steps_done, traj_host, true);
}

// the same loops with the context's source set (pph_sources.hip): coef [nsteps][K] on the host, traj NULL or as the recording
// variants take it
extern "C" int pph_transient_steps_sources_device(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_dev, int nsteps,
                                                  double steady_tol, pph_solve_info* infos, double* norms, int* steps_done,
                                                  double* traj_dev, const double* coef, int64_t K) {
  if (!ctx) return PPH_ERR_INVALID;
  return transient_steps_dev(ctx, cfg, p_dev, nsteps, steady_tol, infos, norms, steps_done, traj_dev, true, coef, K);
}

extern "C" int pph_transient_steps_sources(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_host, int nsteps, double steady_tol,
                                           pph_solve_info* infos, double* norms, int* steps_done, double* traj_host,
                                           const double* coef, int64_t K) {
  if (!ctx) return PPH_ERR_INVALID;
  return transient_steps_host(ctx, cfg, p_host, nsteps, steady_tol, infos, norms, steps_done, traj_host, traj_host != nullptr, true,
                              coef, K);
}
