// Degree-2 Lagrange elements (Q2 quadrilaterals / hexahedra, P2 triangles / tetrahedra) on the structured meshes: local
// node order, reference basis, used by the mesh / assembly kernels (pph_p2.hip) and the error norms (pph_post.hip).
//
// Degree-2 nodes are the points of the lattice refined once: lattice point (I,J,K) -> I + (2nx+1)(J + (2ny+1)K), at
// (I/2nx, J/2ny, K/2nz).  Box (ci,cj,ck) spans lattice points (2ci..2ci+2, 2cj..2cj+2, 2ck..2ck+2); its CG-1 vertex v
// (bits x, y, z of v) is the lattice point (2ci + 2(v&1), 2cj + 2((v>>1)&1), 2ck + 2((v>>2)&1)).
// Local node order of a cell:
//   Q2 quad (9) / hex (27): lattice offset (a, b[, c]) in {0,1,2}^d of the box -> local a + 3b (+ 9c)
//   P2 triangle (6): the cell's three CG-1 vertices (k_dofmap order), then the midpoints of edges 01, 02, 12
//   P2 tetrahedron (10): the four CG-1 vertices (k_dofmap order), then the midpoints of edges 01, 02, 03, 12, 13, 23
// Reference cells: [0,1]^d (nodes at 0, 1/2, 1 per direction) and the unit simplex (vertex 0 at the origin, vertex r at
// e_r); the affine map x = X0 + J xi, J's columns the edges X(1) - X(0), X(2) - X(0) (, X(4) - X(0) for the hex /
// X(3) - X(0) for the tet) between the cell's CG-1 vertices.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PPH_P2_MAXM 27

__host__ __device__ static inline int p2_nodes_per_cell(int kind) {
  return kind == PPH_CELL_QUAD ? 9 : kind == PPH_CELL_TRI ? 6 : kind == PPH_CELL_HEX ? 27 : 10;
}
__host__ __device__ static inline int p2_cells_per_box(int kind) {
  return kind == PPH_CELL_TRI ? 2 : kind == PPH_CELL_TET ? 6 : 1;
}

// CG-1 vertices (box corner ids v = x + 2y + 4z) of sub-cell s of a box: k_dofmap's order
__host__ __device__ static inline int p2_simplex_vertex(int kind, int s, int r) {
  if (kind == PPH_CELL_TRI) {
    const int T[2][3] = {{0, 1, 2}, {1, 3, 2}};
    return T[s][r];
  }
  const int T[6][4] = {{0, 1, 3, 7}, {0, 1, 7, 5}, {0, 5, 7, 4}, {0, 3, 2, 7}, {0, 6, 4, 7}, {0, 2, 6, 7}};
  return T[s][r];
}

// lattice offset (ox, oy, oz) in {0,1,2}^3 inside its box of local node a of sub-cell s
__host__ __device__ static inline void p2_local_offset(int kind, int s, int a, int o[3]) {
  if (kind == PPH_CELL_QUAD || kind == PPH_CELL_HEX) {
    o[0] = a % 3; o[1] = (a / 3) % 3; o[2] = a / 9;
    return;
  }
  const int nv = (kind == PPH_CELL_TRI) ? 3 : 4;
  int p, q;
  if (a < nv) { p = q = a; }
  else if (kind == PPH_CELL_TRI) {
    const int E[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    p = E[a - 3][0]; q = E[a - 3][1];
  } else {
    const int E[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
    p = E[a - 4][0]; q = E[a - 4][1];
  }
  const int vp = p2_simplex_vertex(kind, s, p), vq = p2_simplex_vertex(kind, s, q);
  o[0] = (vp & 1) + (vq & 1);
  o[1] = ((vp >> 1) & 1) + ((vq >> 1) & 1);
  o[2] = ((vp >> 2) & 1) + ((vq >> 2) & 1);
}

// quadratic Lagrange basis on [0,1] with nodes 0, 1/2, 1: value and derivative of function i at t
__host__ __device__ static inline void p2_1d(int i, double t, double* v, double* d) {
  if (i == 0) { *v = (2.0 * t - 1.0) * (t - 1.0); *d = 4.0 * t - 3.0; }
  else if (i == 1) { *v = 4.0 * t * (1.0 - t); *d = 4.0 - 8.0 * t; }
  else { *v = t * (2.0 * t - 1.0); *d = 4.0 * t - 1.0; }
}

// reference basis function a of the cell kind at xi (DIM coordinates): value and reference gradient
template <int KIND>
__host__ __device__ static inline void p2_basis(int a, const double* xi, double* N, double* dN) {
  if constexpr (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_HEX) {
    constexpr int D = (KIND == PPH_CELL_QUAD) ? 2 : 3;
    double v[3], d[3];
    const int ia[3] = {a % 3, (a / 3) % 3, a / 9};
#pragma unroll
    for (int e = 0; e < D; ++e) p2_1d(ia[e], xi[e], &v[e], &d[e]);
    if constexpr (D == 2) {
      *N = v[0] * v[1];
      dN[0] = d[0] * v[1];
      dN[1] = v[0] * d[1];
    } else {
      *N = v[0] * v[1] * v[2];
      dN[0] = d[0] * v[1] * v[2];
      dN[1] = v[0] * d[1] * v[2];
      dN[2] = v[0] * v[1] * d[2];
    }
  } else {
    constexpr int D = (KIND == PPH_CELL_TRI) ? 2 : 3;
    // barycentric lambda_0 = 1 - sum xi, lambda_r = xi_{r-1}; d lambda_0 / d xi_e = -1, d lambda_r / d xi_e = delta
    double lam[4];
    lam[0] = 1.0;
#pragma unroll
    for (int e = 0; e < D; ++e) { lam[e + 1] = xi[e]; lam[0] -= xi[e]; }
    auto dl = [](int r, int e) { return r == 0 ? -1.0 : (r - 1 == e ? 1.0 : 0.0); };
    if (a <= D) {
      *N = lam[a] * (2.0 * lam[a] - 1.0);
#pragma unroll
      for (int e = 0; e < D; ++e) dN[e] = (4.0 * lam[a] - 1.0) * dl(a, e);
    } else {
      int p, q;
      if constexpr (D == 2) {
        const int E[3][2] = {{0, 1}, {0, 2}, {1, 2}};
        p = E[a - 3][0]; q = E[a - 3][1];
      } else {
        const int E[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
        p = E[a - 4][0]; q = E[a - 4][1];
      }
      *N = 4.0 * lam[p] * lam[q];
#pragma unroll
      for (int e = 0; e < D; ++e) dN[e] = 4.0 * (dl(p, e) * lam[q] + lam[p] * dl(q, e));
    }
  }
}

// local indices of the CG-1 vertices that span the affine map (X0 and the ends of J's columns)
__host__ __device__ static inline int p2_frame_node(int kind, int r) {
  if (kind == PPH_CELL_QUAD) { const int F[3] = {0, 2, 6}; return F[r]; }
  if (kind == PPH_CELL_HEX) { const int F[4] = {0, 2, 6, 18}; return F[r]; }
  return r;   // simplices: the vertices come first
}
