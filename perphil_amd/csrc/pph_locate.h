// Point location on the uniform boxes and the CG-1 bases of the four cell kinds: the device code pph_eval.hip (point
// evaluation) and pph_trace.hip (pathlines) share, so that both locate a point and weigh a cell's nodes by the same text.
//
// Location rule.  Per direction e: t_e = x_e n_e (ONE rounding), box index c_e = clamp(floor(t_e), 0, n_e - 1), box-local
// coordinate xi_e = t_e - c_e (exact).  Sub-cells of a box (k_dofmap's order, p2_simplex_vertex):
//   triangles: sub-cell 0 {0,1,2} where xi_x + xi_y <= 1, else sub-cell 1 {1,3,2};
//   Kuhn tetrahedra: the sub-cell whose corners form the path 0 -> .. -> 7 that steps along the axes (a, b, c) in the
//   descending order xi_a >= xi_b >= xi_c; barycentric coordinates 1 - xi_a, xi_a - xi_b, xi_b - xi_c, xi_c along the
//   path, handed to the cell's local vertices in the cell's own order.
// Tie-break: a point on a face shared by several sub-cells of a box goes to the LOWEST sub-cell index; a point on a face
// between two boxes (t_e an integer) goes to the upper box, except on the domain's far boundary.
#pragma once
#include "pph_internal.h"
#include "pph_p2.h"

struct EvalGeo { int n[3]; };   // boxes per direction

// direction e of the point x: box index (as a double: floor's result, NaN -> 0) and the UNCLAMPED box-local coordinate
__device__ static inline double box_locate(double x, int n, double* c_out) {
  const double t = x * (double)n;
  const double c = fmin(fmax(floor(t), 0.0), (double)(n - 1));   // (NaN -> 0)
  *c_out = c;
  return t - c;
}

// Q1 shape function of box corner b (bit e of b: the far end along e) from the 1-D weights w[e] = {1 - xi_e, xi_e}
template <int DIM>
__device__ static inline double q1_shape(const double (*w)[2], int b) {
  double nv = w[0][b & 1] * w[1][(b >> 1) & 1];
  if constexpr (DIM == 3) nv *= w[2][(b >> 2) & 1];
  return nv;
}

// Kuhn sub-cell s: axes (a, b, c) of its path 0 -> 7, and the path position of its local vertex r (= the number of
// set bits of the box corner p2_simplex_vertex(TET, s, r))
__device__ static inline int tet_axis(int s, int k) {
  const int A[6][3] = {{0, 1, 2}, {0, 2, 1}, {2, 0, 1}, {1, 0, 2}, {2, 1, 0}, {1, 2, 0}};
  return A[s][k];
}
__device__ static inline int tet_pos(int s, int r) {
  const int P[6][4] = {{0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 3, 1}, {0, 2, 1, 3}, {0, 2, 1, 3}, {0, 1, 2, 3}};
  return P[s][r];
}

// sub-cell of the box-local point xi, barycentric coordinates lam[r] of the sub-cell's local vertices and their
// (constant) derivatives D[r][e] = d lam_r / d xi_e
template <int KIND>
__device__ static inline int simplex_locate(const double* xi, double* lam, double (*D)[3]) {
  if constexpr (KIND == PPH_CELL_TRI) {
    const bool lower = xi[0] + xi[1] <= 1.0;
    if (lower) {
      lam[0] = 1.0 - xi[0] - xi[1]; lam[1] = xi[0]; lam[2] = xi[1];
      D[0][0] = -1.0; D[0][1] = -1.0; D[1][0] = 1.0; D[1][1] = 0.0; D[2][0] = 0.0; D[2][1] = 1.0;
      return 0;
    }
    lam[0] = 1.0 - xi[1]; lam[1] = xi[0] + xi[1] - 1.0; lam[2] = 1.0 - xi[0];
    D[0][0] = 0.0; D[0][1] = -1.0; D[1][0] = 1.0; D[1][1] = 1.0; D[2][0] = -1.0; D[2][1] = 0.0;
    return 1;
  } else {
    int s = 5;
#pragma unroll
    for (int q = 4; q >= 0; --q)
      if (xi[tet_axis(q, 0)] >= xi[tet_axis(q, 1)] && xi[tet_axis(q, 1)] >= xi[tet_axis(q, 2)]) s = q;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      if (q != s) continue;
      const int a = tet_axis(q, 0), b = tet_axis(q, 1), c = tet_axis(q, 2);
      const double lp[4] = {1.0 - xi[a], xi[a] - xi[b], xi[b] - xi[c], xi[c]};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = tet_pos(q, r);
        lam[r] = lp[k];
#pragma unroll
        for (int e = 0; e < 3; ++e)
          D[r][e] = (k == 0) ? (e == a ? -1.0 : 0.0)
                  : (k == 1) ? (e == a ? 1.0 : (e == b ? -1.0 : 0.0))
                  : (k == 2) ? (e == b ? 1.0 : (e == c ? -1.0 : 0.0))
                             : (e == c ? 1.0 : 0.0);
      }
    }
    return s;
  }
}

// basis values N[b] of the box-local point xi (inside, clamped) in its cell; returns the sub-cell.  The values k_eval_points
// forms, by the same calls in the same order (the transposed evaluation and the point loads of pph_sources.hip).
template <int KIND, int DEG, int NB>
__device__ static inline int adj_basis(const double* xi, double* N) {
  constexpr int DIM = (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_TRI) ? 2 : 3;
  constexpr bool SIMPLEX = (KIND == PPH_CELL_TRI || KIND == PPH_CELL_TET);
  if constexpr (!SIMPLEX) {
    if constexpr (DEG == 1) {
      double w[3][2];
#pragma unroll
      for (int e = 0; e < DIM; ++e) { w[e][0] = 1.0 - xi[e]; w[e][1] = xi[e]; }
#pragma unroll
      for (int b = 0; b < NB; ++b) N[b] = q1_shape<DIM>(w, b);
    } else {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        double d[3];
        p2_basis<KIND>(b, xi, &N[b], d);
      }
    }
    return 0;
  } else {
    double lam[DIM + 1], D[DIM + 1][3];
    const int sub = simplex_locate<KIND>(xi, lam, D);
    if constexpr (DEG == 1) {
#pragma unroll
      for (int b = 0; b < NB; ++b) N[b] = lam[b];
    } else {
      double xr[DIM];   // reference coordinates of pph_p2.h: xr_j = lam_{j+1}
#pragma unroll
      for (int j = 0; j < DIM; ++j) xr[j] = lam[j + 1];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        double d[3];
        p2_basis<KIND>(b, xr, &N[b], d);
      }
    }
    return sub;
  }
}
