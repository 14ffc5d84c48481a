// Element forms a^T K_e b and a^T M_e b of the uniform boxes, matrix-free, and the reduction layout around them: what
// k_dpp_bilinear (pph_adjoint.hip) and k_transient_bilinear (pph_transient_adjoint.hip) share.  pph_adjoint.hip states the
// forms and the determinism rule.
#pragma once
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
static __global__ __launch_bounds__(256) void k_bilinear_sum(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
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
