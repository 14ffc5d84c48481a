// p-multigrid (PPH_PC_PMG): the products of the degree-2 level that sits on top of the CG-1 hierarchy (pph_mg.hip builds
// the hierarchy and runs the cycle; the transfers between the degree-2 level and the CG-1 level on the same cells are the
// h-transfer kernels, because the degree-2 nodes are the CG-1 nodes of the mesh refined once).
//
// With mg_smooth = 2 a cycle passes four times over the degree-2 operator (one Chebyshev product and one residual on the
// way down, the same on the way up) and everything below is a problem eight times smaller, so these passes are the cycle.
// Their rows differ in length by node parity (Q2 hexahedra 125 / 75 / 45 / 27 entries, Q2 quadrilaterals 25 / 15 / 9,
// fewer at the boundary), which a CSR-vector kernel with a fixed number of lanes per row serves badly: eight lanes take
// four steps for a 125-row and leave one lane idle on a 27-row of the same workgroup.  Here the lanes are not bound to
// rows while the matrix is read:
//   1. a workgroup takes a tile of R consecutive rows; its entries are ONE contiguous range of val / col.  The range
//      (start rounded down to a multiple of 4) is cut into quads of four entries and the 256 threads take the quads in turn:
//      every lane issues 16-byte loads (one of columns, two of values), every lane is busy whatever the row lengths are,
//      i.e. a row gets ceil(len / 4) lanes; the four products a x go to LDS;
//   2. R groups of 256 / R lanes add the products of one row each, in a fixed order (strided partial sums, then a
//      shuffle tree): two runs give bitwise equal results;
//   3. lane 0 of a group applies the row's epilogue - the Chebyshev recurrence of the smoother or the (masked) residual.
// Tiles are dealt to the workgroups as k_spmv_wide deals its chunks: one contiguous eighth of the rows per XCD, so that
// the gathers of neighbouring tiles meet in the same L2.
#include "pph_internal.h"

#define PMG_R3 32            // rows per tile, 3D (Q2 hex: 64 entries per row on average -> 2 quads per lane)
#define PMG_R3S 16           // ... the small 3D tile ("pmg_tile_rows" 16): half the LDS, twice the workgroups per compute unit
#define PMG_R2 64            // rows per tile, 2D (Q2 quad: 16 entries per row on average -> 1 quad per lane)
// products of one tile: R * max_row + 3 doubles must fit (checked on the host); 3D rows have at most 125 entries, 2D rows 25
__host__ __device__ constexpr int pmg_cap(int R) { return R == PMG_R2 ? 1664 : (R == PMG_R3 ? 4096 : 2048); }

// MODE 0, smoother step:  t = A d;  r -= t;  d' = c1 d + c2 dinv r;  x += d'    (d' to dnew: neighbours still read d)
// MODE 1, residual:       r = b - A x, 0 where mask is set (mask may be NULL)
template <int R, int MODE>
__global__ __launch_bounds__(256) void k_pmg_level0(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                    const double* __restrict__ val, int64_t nrows, int64_t nnz,
                                                    const double* __restrict__ v /* d or x */,
                                                    const double* __restrict__ dinv, double* __restrict__ r,
                                                    double* __restrict__ dnew, double* __restrict__ x, double c1, double c2,
                                                    const double* __restrict__ b, const uint8_t* __restrict__ mask) {
  constexpr int G = 256 / R;
  constexpr int CAP = pmg_cap(R);
  __shared__ double prod[CAP];
  __shared__ int rel[R + 1];
  const int tid = threadIdx.x;
  const int grp = tid / G, sub = tid % G;
  const int64_t ntiles = (nrows + R - 1) / R;
  const int xcd = blockIdx.x & 7, bx = blockIdx.x >> 3, bpx = gridDim.x >> 3;
  const int64_t tpx = (ntiles + 7) >> 3;
  const int64_t t_begin = (int64_t)xcd * tpx;
  const int64_t t_end = (t_begin + tpx < ntiles) ? t_begin + tpx : ntiles;
  for (int64_t tile = t_begin + bx; tile < t_end; tile += bpx) {
    const int64_t row0 = tile * R;
    const int rows = (int)((nrows - row0 < R) ? nrows - row0 : R);
    const int64_t S = rowptr[row0] & ~(int64_t)3;
    const int64_t E = rowptr[row0 + rows];
    if (tid <= rows) rel[tid] = (int)(rowptr[row0 + tid] - S);
    int span = (int)(E - S);
    if (span > CAP) span = CAP;   // (cannot happen: the host checks R * max_row + 3)
    const int nq = (span + 3) >> 2;
    for (int q = tid; q < nq; q += 256) {
      const int64_t base = S + 4 * (int64_t)q;
      // 16-byte loads; device buffers carry 64 bytes of slack, so the last quad stays inside the allocations
      const int4 c = *reinterpret_cast<const int4*>(col + base);
      const double2 a01 = *reinterpret_cast<const double2*>(val + base);
      const double2 a23 = *reinterpret_cast<const double2*>(val + base + 2);
      const bool k1 = base + 1 < nnz, k2 = base + 2 < nnz, k3 = base + 3 < nnz;   // (base < nnz always)
      const double x0 = v[c.x], x1 = v[k1 ? c.y : 0], x2 = v[k2 ? c.z : 0], x3 = v[k3 ? c.w : 0];
      double2 p01, p23;
      p01.x = a01.x * x0; p01.y = k1 ? a01.y * x1 : 0.0;
      p23.x = k2 ? a23.x * x2 : 0.0; p23.y = k3 ? a23.y * x3 : 0.0;
      *reinterpret_cast<double2*>(&prod[4 * q]) = p01;
      *reinterpret_cast<double2*>(&prod[4 * q + 2]) = p23;
    }
    __syncthreads();
    double sum = 0.0;
    if (grp < rows) {
      int s = rel[grp], e = rel[grp + 1];
      if (e > span) e = span;
      for (int i = s + sub; i < e; i += G) sum += prod[i];
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, G);
    if (sub == 0 && grp < rows) {
      const int64_t row = row0 + grp;
      if (MODE == 0) {
        const double rn = r[row] - sum;
        const double dn = c1 * v[row] + c2 * (dinv[row] * rn);
        r[row] = rn;
        dnew[row] = dn;
        x[row] += dn;
      } else {
        r[row] = (mask && mask[row]) ? 0.0 : b[row] - sum;
      }
    }
    __syncthreads();   // prod / rel are rewritten by the next tile
  }
}

__global__ void k_pmg_zero_masked(double* __restrict__ v, const uint8_t* __restrict__ mask, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (mask[i]) v[i] = 0.0;
}

void pmg_zero_masked(pph_ctx* ctx, double* v, const uint8_t* mask, int64_t n) {
  int64_t g = ceil_div64(n, 256);
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(k_pmg_zero_masked, dim3((int)g), dim3(256), 0, ctx->stream, v, mask, n);
}

static int pmg_rows(const pph_ctx* ctx) {
  return (ctx->mesh.dim == 3) ? (ctx->pmg_tile_rows == PMG_R3S ? PMG_R3S : PMG_R3) : PMG_R2;
}

// the tile kernels serve this operator: plain fp64 CSR on one context whose longest row fits the tile's LDS
bool pmg_level0_ok(const pph_ctx* ctx, const Csr& A) {
  if (!ctx->pmg_fused || !A.val || A.val32 || A.ell.val || A.geom || A.max_row <= 0) return false;
  const int R = pmg_rows(ctx);
  return (int64_t)R * A.max_row + 3 <= pmg_cap(R);
}

static int pmg_grid(const pph_ctx* ctx, int64_t nrows, int R) {
  // as many workgroups as the LDS of the 256 compute units holds tiles (five of 32 KB each), rounded to the eight XCDs
  const int64_t ntiles = ceil_div64(nrows, R);
  const int64_t cap = 256 * (int64_t)(160 * 1024 / (pmg_cap(R) * 8 + 512));
  int64_t g = ntiles < cap ? ntiles : cap;
  g = (g + 7) / 8 * 8;
  return (int)(g < 8 ? 8 : g);
}

// bytes one pass moves per the matrix stream (12 per entry, 8 per row pointer) and the vectors of its epilogue
static void pmg_account(pph_ctx* ctx, const Csr& A, double vec_bytes_per_row) {
  const double bytes = 12.0 * (double)A.nnz + (8.0 + vec_bytes_per_row) * (double)A.nrows;
  ctx->n_pmg_pass++;
  ctx->pmg_bytes += bytes;
}

#define PMG_LAUNCH(RR, MODE, ...)                                                                                          \
  hipLaunchKernelGGL((k_pmg_level0<RR, MODE>), dim3(pmg_grid(ctx, A.nrows, RR)), dim3(256), 0, ctx->stream, A.rowptr, A.col, \
                     A.val, A.nrows, A.nnz, __VA_ARGS__)
#define PMG_DISPATCH(MODE, ...)                                 \
  switch (pmg_rows(ctx)) {                                      \
    case PMG_R3: PMG_LAUNCH(PMG_R3, MODE, __VA_ARGS__); break;  \
    case PMG_R3S: PMG_LAUNCH(PMG_R3S, MODE, __VA_ARGS__); break; \
    default: PMG_LAUNCH(PMG_R2, MODE, __VA_ARGS__); break;      \
  }

void pmg_cheb_step(pph_ctx* ctx, const Csr& A, const double* dinv, const double* d, double* dnew, double* r, double* x,
                   double c1, double c2) {
  PMG_DISPATCH(0, d, dinv, r, dnew, x, c1, c2, (const double*)nullptr, (const uint8_t*)nullptr);
  pmg_account(ctx, A, 8.0 /* d */ + 8.0 /* dinv */ + 16.0 /* r */ + 8.0 /* d' */ + 16.0 /* x */);
}

void pmg_resid(pph_ctx* ctx, const Csr& A, const double* x, const double* b, const uint8_t* mask, double* r) {
  PMG_DISPATCH(1, x, (const double*)nullptr, r, (double*)nullptr, (double*)nullptr, 0.0, 0.0, b, mask);
  pmg_account(ctx, A, 8.0 /* x */ + 8.0 /* b */ + 8.0 /* r */ + (mask ? 1.0 : 0.0));
}
