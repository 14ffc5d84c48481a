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

#define BL_MAX_BLOCKS 2048   // partial sums per quantity

struct BlGeo {
  double cd[3];    // n_d^2 |cell|: weight of direction d's derivative product
  double vol;      // |cell| = |box| / cells per box
};
struct BlTab { double m[10][10]; };   // P2 simplices: int phi_a phi_b / |cell|

template <int KIND, int DEG>
struct BlCell {
  static constexpr int DIM = (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_TRI) ? 2 : 3;
  static constexpr bool SIMPLEX = (KIND == PPH_CELL_TRI || KIND == PPH_CELL_TET);
  static constexpr int NB = (DEG == 2) ? ((KIND == PPH_CELL_QUAD) ? 9 : (KIND == PPH_CELL_TRI) ? 6 : (KIND == PPH_CELL_HEX) ? 27 : 10)
                                       : (SIMPLEX ? DIM + 1 : (1 << DIM));
  static constexpr int CPB = (KIND == PPH_CELL_TRI) ? 2 : (KIND == PPH_CELL_TET) ? 6 : 1;   // cells per box
  static constexpr bool ONE_PASS = (4 * NB <= 64);   // the four fields of a cell fit in registers beside the work
};

// sum over the workgroup (256 threads), fixed order; every thread gets it
__device__ static inline double bl_block_sum(double v, double* lds) {
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

// out[q] = sum of part[q * BL_MAX_BLOCKS + i], i < nblocks; one workgroup per quantity q
__global__ __launch_bounds__(256) void k_bilinear_sum(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  __shared__ double lds[256];
  const double* p = part + (int64_t)blockIdx.x * BL_MAX_BLOCKS;
  double v = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) v += p[i];
  v = bl_block_sum(v, lds);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// 1-D stiffness / mass matrices of the tensor-product elements on [0, 1]
template <int DEG>
__device__ static inline double bl_s1(int i, int j) {
  if constexpr (DEG == 1) return i == j ? 1.0 : -1.0;
  else return (i == 1 && j == 1) ? 16.0 / 3.0 : ((i == 1 || j == 1) ? -8.0 / 3.0 : (i == j ? 7.0 / 3.0 : 1.0 / 3.0));
}
template <int DEG>
__device__ static inline double bl_m1(int i, int j) {
  if constexpr (DEG == 1) return i == j ? 1.0 / 3.0 : 1.0 / 6.0;
  else return (i == 1 && j == 1) ? 16.0 / 30.0 : ((i == 1 || j == 1) ? 2.0 / 30.0 : (i == j ? 4.0 / 30.0 : -1.0 / 30.0));
}

// out = (S or Mm along direction e, identity along the others) in
template <int DEG, int NB, bool STIFF>
__device__ static inline void bl_axis(const double* in, double* out, int e) {
  constexpr int P = DEG + 1;
  const int stride = (e == 0) ? 1 : (e == 1 ? P : P * P);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int ie = (b / stride) % P, base = b - ie * stride;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) s += (STIFF ? bl_s1<DEG>(ie, j) : bl_m1<DEG>(ie, j)) * in[base + j * stride];
    out[b] = s;
  }
}

template <int NB>
__device__ static inline double bl_dot(const double* a, const double* b) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NB; ++i) s += a[i] * b[i];
  return s;
}

// the vertices (positions in the cell's vertex list) of sub-cell `sub`'s edge along axis d, lower end first
template <int KIND, int DIM>
__device__ static inline void bl_axis_edge(int sub, int d, int* lo, int* up) {
  *lo = 0; *up = 0;
#pragma unroll
  for (int r = 0; r <= DIM; ++r)
#pragma unroll
    for (int s = 0; s <= DIM; ++s) {
      const int vr = p2_simplex_vertex(KIND, sub, r), vs = p2_simplex_vertex(KIND, sub, s);
      if (vs == (vr | (1 << d)) && vr != vs) { *lo = r; *up = s; }
    }
}

// a^T K_e b of one cell (tensor cells: the box; simplices: sub-cell `sub`); a(k), b(k): the two sides' value at local node k.
// Hexahedra: one z layer of the p side at a time goes through the in-plane factors, the z factors are applied inside the dot
// product with the lambda side - two box-sized intermediates (U, T), one layer of everything else.
template <int KIND, int DEG, class FA, class FB>
__device__ static inline double bl_stiff(FA a, FB b, const BlGeo& g, int sub) {
  using C = BlCell<KIND, DEG>;
  constexpr int DIM = C::DIM, NB = C::NB;
  if constexpr (!C::SIMPLEX) {
    constexpr int P = DEG + 1, P2 = P * P;
    double U[NB], T[(DIM == 3) ? NB : 1];
#pragma unroll
    for (int c = 0; c < (DIM == 3 ? P : 1); ++c) {
      double bc[P2], mx[P2], sx[P2], t[P2];
#pragma unroll
      for (int k = 0; k < P2; ++k) bc[k] = b(c * P2 + k);
      bl_axis<DEG, P2, false>(bc, mx, 0);
      bl_axis<DEG, P2, true>(bc, sx, 0);
      bl_axis<DEG, P2, false>(sx, t, 1);    // My Sx b
#pragma unroll
      for (int k = 0; k < P2; ++k) U[c * P2 + k] = g.cd[0] * t[k];
      bl_axis<DEG, P2, true>(mx, t, 1);     // Sy Mx b
#pragma unroll
      for (int k = 0; k < P2; ++k) U[c * P2 + k] += g.cd[1] * t[k];
      if constexpr (DIM == 3) bl_axis<DEG, P2, false>(mx, &T[c * P2], 1);   // My Mx b
    }
    double acc = 0.0;
    if constexpr (DIM == 2) {
#pragma unroll
      for (int k = 0; k < NB; ++k) acc += a(k) * U[k];
    } else {
#pragma unroll
      for (int c = 0; c < P; ++c)
#pragma unroll
        for (int k = 0; k < P2; ++k) {
          double vm = 0.0, vs = 0.0;   // row c of Mz (c_x My Sx + c_y Sy Mx) b and of Sz My Mx b
#pragma unroll
          for (int c2 = 0; c2 < P; ++c2) { vm += bl_m1<DEG>(c, c2) * U[c2 * P2 + k]; vs += bl_s1<DEG>(c, c2) * T[c2 * P2 + k]; }
          acc += a(c * P2 + k) * (vm + g.cd[2] * vs);
        }
    }
    return acc;
  } else {
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      int lo, up;
      bl_axis_edge<KIND, DIM>(sub, d, &lo, &up);
      if constexpr (DEG == 1) {
        acc += g.cd[d] * ((a(up) - a(lo)) * (b(up) - b(lo)));
      } else {
        double sa = 0.0, sb = 0.0, sab = 0.0;
#pragma unroll
        for (int v = 0; v <= DIM; ++v) {   // the edge derivative at vertex v (reference coordinates xr_j = lambda_{j+1})
          double xr[DIM];
#pragma unroll
          for (int j = 0; j < DIM; ++j) xr[j] = (j + 1 == v) ? 1.0 : 0.0;
          double ga = 0.0, gb = 0.0;
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            double nv, dn[3];
            p2_basis<KIND>(k, xr, &nv, dn);
            double along = 0.0;   // reference vertex r > 0 is e_{r-1}, vertex 0 the origin
#pragma unroll
            for (int j = 0; j < DIM; ++j) along += (j + 1 == up ? dn[j] : 0.0) - (j + 1 == lo ? dn[j] : 0.0);
            if (along != 0.0) { ga += along * a(k); gb += along * b(k); }
          }
          sa += ga; sb += gb; sab += ga * gb;
        }
        acc += g.cd[d] * ((sa * sb + sab) / (double)((DIM + 1) * (DIM + 2)));
      }
    }
    return acc;
  }
}

// a^T M_e b of one cell
template <int KIND, int DEG, class FA, class FB>
__device__ static inline double bl_mass(FA a, FB b, const BlGeo& g, const BlTab& tab) {
  using C = BlCell<KIND, DEG>;
  constexpr int DIM = C::DIM, NB = C::NB;
  if constexpr (!C::SIMPLEX) {
    constexpr int P = DEG + 1, P2 = P * P;
    double T[NB];
#pragma unroll
    for (int c = 0; c < (DIM == 3 ? P : 1); ++c) {
      double bc[P2], mx[P2];
#pragma unroll
      for (int k = 0; k < P2; ++k) bc[k] = b(c * P2 + k);
      bl_axis<DEG, P2, false>(bc, mx, 0);
      bl_axis<DEG, P2, false>(mx, &T[c * P2], 1);
    }
    double acc = 0.0;
    if constexpr (DIM == 2) {
#pragma unroll
      for (int k = 0; k < NB; ++k) acc += a(k) * T[k];
    } else {
#pragma unroll
      for (int c = 0; c < P; ++c)
#pragma unroll
        for (int k = 0; k < P2; ++k) {
          double vm = 0.0;
#pragma unroll
          for (int c2 = 0; c2 < P; ++c2) vm += bl_m1<DEG>(c, c2) * T[c2 * P2 + k];
          acc += a(c * P2 + k) * vm;
        }
    }
    return g.vol * acc;
  } else if constexpr (DEG == 1) {
    double sa = 0.0, sb = 0.0, sab = 0.0;
#pragma unroll
    for (int r = 0; r < NB; ++r) { sa += a(r); sb += b(r); sab += a(r) * b(r); }
    return g.vol * ((sa * sb + sab) / (double)((DIM + 1) * (DIM + 2)));
  } else {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < NB; ++j) s += tab.m[i][j] * b(j);
      acc += a(i) * s;
    }
    return g.vol * acc;
  }
}

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

// int phi_a phi_b / |cell| of the P2 basis of pph_p2.h on a simplex of dimension D, from the barycentric integrals
static void bl_p2_mass_table(int D, BlTab* tab) {
  const int nv = D + 1, nb = (D == 2) ? 6 : 10;
  const int E2[3][2] = {{0, 1}, {0, 2}, {1, 2}};
  const int E3[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
  struct Mono { double c; int e[4]; };
  auto basis = [&](int a, Mono out[2]) -> int {   // phi_r = 2 lambda_r^2 - lambda_r ; phi_pq = 4 lambda_p lambda_q
    for (int k = 0; k < 2; ++k) for (int i = 0; i < 4; ++i) out[k].e[i] = 0;
    if (a < nv) {
      out[0].c = 2.0; out[0].e[a] = 2;
      out[1].c = -1.0; out[1].e[a] = 1;
      return 2;
    }
    const int* pq = (D == 2) ? E2[a - nv] : E3[a - nv];
    out[0].c = 4.0; out[0].e[pq[0]] = 1; out[0].e[pq[1]] = 1;
    return 1;
  };
  auto fact = [](int k) { double f = 1.0; for (int i = 2; i <= k; ++i) f *= i; return f; };
  for (int a = 0; a < 10; ++a) for (int b = 0; b < 10; ++b) tab->m[a][b] = 0.0;
  for (int a = 0; a < nb; ++a)
    for (int b = 0; b < nb; ++b) {
      Mono ma[2], mb[2];
      const int na = basis(a, ma), nbm = basis(b, mb);
      double s = 0.0;
      for (int i = 0; i < na; ++i)
        for (int j = 0; j < nbm; ++j) {
          double num = fact(D);
          int tot = D;
          for (int k = 0; k < nv; ++k) { num *= fact(ma[i].e[k] + mb[j].e[k]); tot += ma[i].e[k] + mb[j].e[k]; }
          s += ma[i].c * mb[j].c * num / fact(tot);
        }
      tab->m[a][b] = s;
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
