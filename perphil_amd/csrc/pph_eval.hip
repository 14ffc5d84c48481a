// Point evaluation: values (and gradients) of a finite-element function at arbitrary points of the unit square / cube.
//
// Replaces Firedrake's Function.at (what the reference's slice_along_x samples, src/perphil/utils/postprocessing.py:66-86)
// on the structured meshes, for CG-1 and degree-2 (pph_p2.h) fields on all four cell kinds.  One thread per point,
// grid-stride; no search structure: the meshes are uniform boxes, so locating a point is arithmetic.
//
// Location rule (the code is pph_locate.h's, shared with pph_trace.hip).  Per direction e: t_e = x_e n_e (ONE rounding; everything after it is exact up to the basis evaluation),
// box index c_e = clamp(floor(t_e), 0, n_e - 1), box-local coordinate xi_e = t_e - c_e (exact).  The point is OUTSIDE when
// some xi_e lies outside [-tol, 1 + tol] (tol in box-local units; NaN coordinates are outside): every output of the point
// is NaN and the point is counted.  An inside point is clamped to [0, 1].
// Sub-cells of a box (k_dofmap's order, p2_simplex_vertex):
//   triangles: sub-cell 0 {0,1,2} where xi_x + xi_y <= 1, else sub-cell 1 {1,3,2};
//   Kuhn tetrahedra: the sub-cell whose corners form the path 0 -> .. -> 7 that steps along the axes (a, b, c) in the
//   descending order xi_a >= xi_b >= xi_c; barycentric coordinates 1 - xi_a, xi_a - xi_b, xi_b - xi_c, xi_c along the
//   path, handed to the cell's local vertices in the cell's own order.
// Tie-break: a point on a face shared by several sub-cells of a box goes to the LOWEST sub-cell index; a point on a face
// between two boxes (t_e an integer) goes to the upper box, except on the domain's far boundary.  Values are continuous
// across faces, so the choice shows in gradients only.
// Gradients: the cells are affine, J^-T is the diagonal scaling by n_e (of the reference-simplex gradient carried to the
// box's axes for simplices).
//
// Components: u[node * ncomp + c] (node-major, the CG-1 vector space's layout; a scalar field is ncomp = 1).  The point is
// located and the basis evaluated once, then reused for every component.  No LDS: every thread gathers its own cell.
#include "pph_internal.h"
#include "pph_locate.h"
#include "pph_p2.h"
#include <cmath>

template <int KIND, int DEG, bool GRAD>
__global__ __launch_bounds__(256) void k_eval_points(const int32_t* __restrict__ cells, const double* __restrict__ u,
                                                     int ncomp, const double* __restrict__ x, int64_t m, EvalGeo g,
                                                     double tol, double* __restrict__ val, double* __restrict__ grad,
                                                     unsigned long long* __restrict__ n_outside) {
  constexpr int DIM = (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_TRI) ? 2 : 3;
  constexpr bool SIMPLEX = (KIND == PPH_CELL_TRI || KIND == PPH_CELL_TET);
  constexpr int NB = (DEG == 2) ? ((KIND == PPH_CELL_QUAD) ? 9 : (KIND == PPH_CELL_TRI) ? 6 : (KIND == PPH_CELL_HEX) ? 27 : 10)
                                : (SIMPLEX ? DIM + 1 : (1 << DIM));
  constexpr int CPB = (KIND == PPH_CELL_TRI) ? 2 : (KIND == PPH_CELL_TET) ? 6 : 1;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  unsigned long long outside = 0;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
    double xi[3] = {0.0, 0.0, 0.0};
    int64_t box = 0, stride = 1;
    bool out = false;
#pragma unroll
    for (int e = 0; e < DIM; ++e) {
      double c;
      const double s = box_locate(x[p * DIM + e], g.n[e], &c);
      out = out || !(s >= -tol && s <= 1.0 + tol);
      xi[e] = fmin(fmax(s, 0.0), 1.0);
      box += stride * (int64_t)c;
      stride *= g.n[e];
    }
    if (out) {
      ++outside;
      for (int c = 0; c < ncomp; ++c) {
        val[p * ncomp + c] = qnan;
        if constexpr (GRAD) {
#pragma unroll
          for (int e = 0; e < DIM; ++e) grad[(p * ncomp + c) * DIM + e] = qnan;
        }
      }
      continue;
    }
    double N[NB], dN[GRAD ? NB : 1][3];   // basis and its derivatives along the box's axes (box-local units)
    int sub = 0;
    if constexpr (!SIMPLEX) {
      if constexpr (DEG == 1) {
        double w[3][2];
#pragma unroll
        for (int e = 0; e < DIM; ++e) { w[e][0] = 1.0 - xi[e]; w[e][1] = xi[e]; }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          N[b] = q1_shape<DIM>(w, b);
          if constexpr (GRAD) {
#pragma unroll
            for (int e = 0; e < DIM; ++e) {
              double d = ((b >> e) & 1) ? 1.0 : -1.0;
#pragma unroll
              for (int f = 0; f < DIM; ++f)
                if (f != e) d *= w[f][(b >> f) & 1];
              dN[b][e] = d;
            }
          }
        }
      } else {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          double nv, d[3];
          p2_basis<KIND>(b, xi, &nv, d);
          N[b] = nv;
          if constexpr (GRAD) {
#pragma unroll
            for (int e = 0; e < DIM; ++e) dN[b][e] = d[e];
          }
        }
      }
    } else {
      double lam[DIM + 1], D[DIM + 1][3];
      sub = simplex_locate<KIND>(xi, lam, D);
      if constexpr (DEG == 1) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          N[b] = lam[b];
          if constexpr (GRAD) {
#pragma unroll
            for (int e = 0; e < DIM; ++e) dN[b][e] = D[b][e];
          }
        }
      } else {
        double xr[DIM];   // reference coordinates of pph_p2.h: xr_j = lam_{j+1}
#pragma unroll
        for (int j = 0; j < DIM; ++j) xr[j] = lam[j + 1];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          double nv, d[3];
          p2_basis<KIND>(b, xr, &nv, d);
          N[b] = nv;
          if constexpr (GRAD) {
#pragma unroll
            for (int e = 0; e < DIM; ++e) {
              double a = d[0] * D[1][e];
#pragma unroll
              for (int j = 1; j < DIM; ++j) a += d[j] * D[j + 1][e];
              dN[b][e] = a;
            }
          }
        }
      }
    }
    const int32_t* cn = cells + (box * CPB + sub) * NB;
    int32_t nd[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) nd[b] = cn[b];
    for (int c = 0; c < ncomp; ++c) {
      double v = 0.0, gr[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const double ub = u[(int64_t)nd[b] * ncomp + c];
        v += N[b] * ub;
        if constexpr (GRAD) {
#pragma unroll
          for (int e = 0; e < DIM; ++e) gr[e] += dN[b][e] * ub;
        }
      }
      val[p * ncomp + c] = v;
      if constexpr (GRAD) {
#pragma unroll
        for (int e = 0; e < DIM; ++e) grad[(p * ncomp + c) * DIM + e] = gr[e] * (double)g.n[e];
      }
    }
  }
  // the total of outside points: one atomic per wave that has any
  for (int o = 32; o > 0; o >>= 1) outside += __shfl_down(outside, o, 64);
  if ((threadIdx.x & 63) == 0 && outside) atomicAdd(n_outside, outside);
}

template <int KIND, int DEG>
static void eval_launch2(pph_ctx* ctx, int grid, const int32_t* cells, const double* u, int ncomp, const double* x, int64_t m,
                         EvalGeo g, double tol, double* val, double* grad, unsigned long long* cnt) {
  if (grad)
    hipLaunchKernelGGL((k_eval_points<KIND, DEG, true>), dim3(grid), dim3(256), 0, ctx->stream, cells, u, ncomp, x, m, g, tol, val, grad, cnt);
  else
    hipLaunchKernelGGL((k_eval_points<KIND, DEG, false>), dim3(grid), dim3(256), 0, ctx->stream, cells, u, ncomp, x, m, g, tol, val, grad, cnt);
}

template <int KIND>
static void eval_launch(pph_ctx* ctx, int degree, int grid, const int32_t* cells, const double* u, int ncomp, const double* x,
                        int64_t m, EvalGeo g, double tol, double* val, double* grad, unsigned long long* cnt) {
  if (degree == 2) eval_launch2<KIND, 2>(ctx, grid, cells, u, ncomp, x, m, g, tol, val, grad, cnt);
  else eval_launch2<KIND, 1>(ctx, grid, cells, u, ncomp, x, m, g, tol, val, grad, cnt);
}

// device memory of one call: released by the entry point whichever way the call ends
struct EvalBufs {
  DevBuf<double> u, x, v, gr;
  DevBuf<unsigned long long> cnt;
  unsigned long long h = 0;   // host copy of the count (lives until release(): hipFree waits for the copy on an error path)
  void release() { u.release(); x.release(); v.release(); gr.release(); cnt.release(); }
};

// device arrays in, device arrays out: enqueues the kernel and the copy of the count to b.h on the context stream
// (the caller synchronises before it reads b.h)
static int eval_enqueue(pph_ctx* ctx, EvalBufs& b, const double* u, int ncomp, const double* x, int64_t m, double tol,
                        double* val, double* grad) {
  const MeshData& ms = ctx->mesh;
  PPH_TRY(b.cnt.alloc(ctx, 1));
  unsigned long long* cnt = b.cnt.p;
  PPH_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), ctx->stream));
  EvalGeo g;
  g.n[0] = ms.nx; g.n[1] = ms.ny; g.n[2] = (ms.dim == 3) ? ms.nzl : 1;
  const int64_t nb = ceil_div64(m, 256);
  const int grid = (int)(nb < 8192 ? nb : 8192);
  if (m > 0) {
    if (ms.kind == PPH_CELL_QUAD) eval_launch<PPH_CELL_QUAD>(ctx, ms.degree, grid, ms.cells.p, u, ncomp, x, m, g, tol, val, grad, cnt);
    else if (ms.kind == PPH_CELL_TRI) eval_launch<PPH_CELL_TRI>(ctx, ms.degree, grid, ms.cells.p, u, ncomp, x, m, g, tol, val, grad, cnt);
    else if (ms.kind == PPH_CELL_HEX) eval_launch<PPH_CELL_HEX>(ctx, ms.degree, grid, ms.cells.p, u, ncomp, x, m, g, tol, val, grad, cnt);
    else eval_launch<PPH_CELL_TET>(ctx, ms.degree, grid, ms.cells.p, u, ncomp, x, m, g, tol, val, grad, cnt);
    PPH_HIP(ctx, hipGetLastError());
  }
  PPH_HIP(ctx, hipMemcpyAsync(&b.h, cnt, sizeof(b.h), hipMemcpyDeviceToHost, ctx->stream));
  return PPH_OK;
}

static int eval_check(pph_ctx* ctx, const char* who, const void* nodal, int ncomp, const void* x, int64_t m, double tol,
                      const void* val, const int64_t* n_outside) {
  PPH_REQUIRE(ctx, ctx->mesh_ok, "%s before pph_mesh_build", who);
  PPH_REQUIRE(ctx, ctx->world == 1, "point evaluation is implemented for single-context meshes");
  PPH_REQUIRE(ctx, nodal && n_outside && m >= 0 && (m == 0 || (x && val)), "%s: NULL buffer or negative point count", who);
  PPH_REQUIRE(ctx, ncomp >= 1, "%s: ncomp must be at least 1, got %d", who, ncomp);
  PPH_REQUIRE(ctx, tol >= 0.0 && tol < 0.5, "%s: tol must be in [0, 0.5) box-local units", who);
  return PPH_OK;
}

static int eval_host(pph_ctx* ctx, EvalBufs& b, const double* nodal_host, int ncomp, const double* x_host, int64_t m, double tol,
                     double* val_host, double* grad_host, int64_t* n_outside) {
  const MeshData& ms = ctx->mesh;
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nu = (size_t)ms.n * ncomp, nx = (size_t)m * ms.dim, nv = (size_t)m * ncomp;
  PPH_TRY(b.u.alloc(ctx, nu));
  PPH_TRY(b.x.alloc(ctx, nx));
  PPH_TRY(b.v.alloc(ctx, nv));
  if (grad_host) PPH_TRY(b.gr.alloc(ctx, nv * ms.dim));
  PPH_HIP(ctx, hipMemcpyAsync(b.u.p, nodal_host, sizeof(double) * nu, hipMemcpyHostToDevice, ctx->stream));
  if (m > 0) PPH_HIP(ctx, hipMemcpyAsync(b.x.p, x_host, sizeof(double) * nx, hipMemcpyHostToDevice, ctx->stream));
  PPH_TRY(eval_enqueue(ctx, b, b.u.p, ncomp, b.x.p, m, tol, b.v.p, grad_host ? b.gr.p : nullptr));
  if (m > 0) {
    PPH_HIP(ctx, hipMemcpyAsync(val_host, b.v.p, sizeof(double) * nv, hipMemcpyDeviceToHost, ctx->stream));
    if (grad_host)
      PPH_HIP(ctx, hipMemcpyAsync(grad_host, b.gr.p, sizeof(double) * nv * ms.dim, hipMemcpyDeviceToHost, ctx->stream));
  }
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *n_outside = (int64_t)b.h;
  return PPH_OK;
}

static int eval_device(pph_ctx* ctx, EvalBufs& b, const double* nodal_dev, int ncomp, const double* x_dev, int64_t m, double tol,
                       double* val_dev, double* grad_dev, int64_t* n_outside) {
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  PPH_TRY(eval_enqueue(ctx, b, nodal_dev, ncomp, x_dev, m, tol, val_dev, grad_dev));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the count is a host result)
  *n_outside = (int64_t)b.h;
  return PPH_OK;
}

extern "C" int pph_eval_points(pph_ctx* ctx, const double* nodal_host, int ncomp, const double* x_host, int64_t m, double tol,
                               double* val_host, double* grad_host, int64_t* n_outside) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(eval_check(ctx, "pph_eval_points", nodal_host, ncomp, x_host, m, tol, val_host, n_outside));
  EvalBufs b;
  const int st = eval_host(ctx, b, nodal_host, ncomp, x_host, m, tol, val_host, grad_host, n_outside);
  b.release();
  return st;
}

extern "C" int pph_eval_points_device(pph_ctx* ctx, const double* nodal_dev, int ncomp, const double* x_dev, int64_t m,
                                      double tol, double* val_dev, double* grad_dev, int64_t* n_outside) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(eval_check(ctx, "pph_eval_points_device", nodal_dev, ncomp, x_dev, m, tol, val_dev, n_outside));
  EvalBufs b;
  const int st = eval_device(ctx, b, nodal_dev, ncomp, x_dev, m, tol, val_dev, grad_dev, n_outside);
  b.release();
  return st;
}
