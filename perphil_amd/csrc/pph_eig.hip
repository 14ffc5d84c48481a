// K-EIG: the two extreme eigenvalues of a symmetric operator of the context by plain Lanczos on the device - what the
// reference's condition-number studies (src/perphil/solvers/conditioning.py:105-218: dense SVD / ARPACK of the exported
// matrix on the host) need of an SPD matrix, without the matrix leaving the GPU.
//
// One step j is four launches: the product w = A v (la_spmv: the kernel pph_spmv would run), k_lanczos_dot (partial sums of
// v.w), k_lanczos_update (alpha_j from the partial sums, r = w - alpha_j v - beta_{j-1} v_prev over v_prev's buffer, partial
// sums of r.r) and k_lanczos_scale (beta_j from those, v_next = r / beta_j).  alpha and beta travel from kernel to kernel
// through device memory; the host reads them every `check_every` steps only (one copy, one synchronisation) and decides on
// the tridiagonal matrix they form.  No reorthogonalisation: the extreme Ritz values converge long before the loss of
// orthogonality matters, and the copies ("ghosts") it produces later repeat eigenvalues, they do not move them.
//
// Why v.w is not taken from the product kernel (la_spmv_dot): its partial sums follow that kernel's grid and row order, and
// those differ between the product paths (stored stencil-ELL values, row-dictionary walk, CSR).  The products themselves are
// bitwise equal on the first two; with a dot of its own - one grid, one order, whatever the product - so is the whole
// iteration: same alpha, beta, step count and estimates on either path.  The price is one more pass over two vectors per step.
// Reductions run in a fixed order (no floating-point atomics): two calls give the same bits.
#include "pph_internal.h"

#include <math.h>
#include <string.h>

#define EIG_BLOCKS 1024     // grid cap of the vector kernels: 1024 blocks x 256 threads x 2 rows per pass (<= PPH_PART_STRIDE partial sums)
#define EIG_PART_AREA 8     // partial sums of v.w in this area of ctx->scal, those of r.r in the next (as k_cg_update_dev's: behind the products')
#define EIG_BREAKDOWN 1e-13

static int eig_grid(int64_t n) {
  int64_t b = ceil_div64((n + 1) / 2, 256);
  if (b < 1) b = 1;
  if (b > EIG_BLOCKS) b = EIG_BLOCKS;
  return (int)b;
}

__device__ inline double eig_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// sum over the 256-thread workgroup; result valid in thread 0
__device__ inline double eig_block_sum(double v, double* lds) {
  v = eig_wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds[w] = v;
  __syncthreads();
  if (w == 0) {
    v = (lane < 4) ? lds[lane] : 0.0;
    v = eig_wave_sum(v);
  }
  return v;
}

// the sum k_reduce_final (pph_la.hip) forms of n partial sums, in its order, in every thread of the block
__device__ inline double eig_total_of_partials(const double* __restrict__ part, int n, double* lds) {
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) v += part[i];
  v = eig_block_sum(v, lds);
  __syncthreads();
  if (threadIdx.x == 0) lds[0] = v;
  __syncthreads();
  v = lds[0];
  __syncthreads();
  return v;
}

// rows in pairs (one 16-byte access per vector and lane), grid-stride; an odd last row is handled by thread 0 of block 0
#define EIG_PAIR_LOOP(p, n) \
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < ((n) >> 1); p += (int64_t)gridDim.x * 256)
#define EIG_HAS_TAIL(n) (((n) & 1) && blockIdx.x == 0 && threadIdx.x == 0)

__device__ inline double eig_hash(int64_t i) {   // k_fill_pattern's values (pph_api.hip): in (-1, 1), a function of the row only
  unsigned long long h = (unsigned long long)i * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
  h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
  return (double)(h >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// start vector (not yet normalised) and the partial sums of its square
__global__ __launch_bounds__(256) void k_eig_start(double* __restrict__ v, int64_t n, double* __restrict__ part) {
  __shared__ double lds[4];
  double acc = 0.0;
  EIG_PAIR_LOOP(p, n) {
    const double a = eig_hash(2 * p), b = eig_hash(2 * p + 1);
    sell_st2(v + 2 * p, a, b);
    acc += a * a + b * b;
  }
  if (EIG_HAS_TAIL(n)) {
    const double a = eig_hash(n - 1);
    v[n - 1] = a;
    acc += a * a;
  }
  acc = eig_block_sum(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// partial sums of y.y
__global__ __launch_bounds__(256) void k_eig_sumsq(const double* __restrict__ y, int64_t n, double* __restrict__ part) {
  __shared__ double lds[4];
  double acc = 0.0;
  EIG_PAIR_LOOP(p, n) {
    double a, b;
    sell_ld2(y + 2 * p, a, b);
    acc += a * a + b * b;
  }
  if (EIG_HAS_TAIL(n)) acc += y[n - 1] * y[n - 1];
  acc = eig_block_sum(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// partial sums of v.w
__global__ __launch_bounds__(256) void k_lanczos_dot(const double* __restrict__ v, const double* __restrict__ w, int64_t n,
                                                     double* __restrict__ part) {
  __shared__ double lds[4];
  double acc = 0.0;
  EIG_PAIR_LOOP(p, n) {
    double v0, v1, w0, w1;
    sell_ld2(v + 2 * p, v0, v1);
    sell_ld2(w + 2 * p, w0, w1);
    acc += v0 * w0 + v1 * w1;
  }
  if (EIG_HAS_TAIL(n)) acc += v[n - 1] * w[n - 1];
  acc = eig_block_sum(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// alpha = sum of k_lanczos_dot's partial sums of v.w (every block, k_reduce_final's order); r = w - alpha v - beta v_prev written
// over v_prev; partial sums of r.r; block 0 stores alpha.  beta_prev null: first step, v_prev is not read.
// VEC (second pass): also y_lo += s_lo v, y_hi += s_hi v with this step's components of the two Ritz vectors of T.
// Plain IEEE arithmetic throughout: the steps enqueued behind a breakdown carry infinities and NaNs and nobody reads them.
template <bool VEC>
__global__ __launch_bounds__(256) void k_lanczos_update(const double* __restrict__ w, const double* __restrict__ v,
                                                        double* __restrict__ vprev, int64_t n,
                                                        const double* __restrict__ part_in, int n_in,
                                                        const double* __restrict__ beta_prev, double* __restrict__ alpha_out,
                                                        double* __restrict__ part_out, double* __restrict__ ylo,
                                                        double* __restrict__ yhi, const double* __restrict__ slo,
                                                        const double* __restrict__ shi) {
  __shared__ double lds[4];
  const double alpha = eig_total_of_partials(part_in, n_in, lds);
  const bool first = beta_prev == nullptr;
  const double beta = first ? 0.0 : *beta_prev;
  if (blockIdx.x == 0 && threadIdx.x == 0) *alpha_out = alpha;
  double cl = 0.0, ch = 0.0;
  if (VEC) { cl = *slo; ch = *shi; }
  double acc = 0.0;
  EIG_PAIR_LOOP(p, n) {
    const int64_t i = 2 * p;
    double w0, w1, v0, v1, q0 = 0.0, q1 = 0.0;
    sell_ld2(w + i, w0, w1);
    sell_ld2(v + i, v0, v1);
    if (!first) sell_ld2(vprev + i, q0, q1);
    const double r0 = first ? w0 - alpha * v0 : w0 - alpha * v0 - beta * q0;
    const double r1 = first ? w1 - alpha * v1 : w1 - alpha * v1 - beta * q1;
    sell_st2(vprev + i, r0, r1);
    acc += r0 * r0 + r1 * r1;
    if (VEC) {
      double a0, a1;
      sell_ld2(ylo + i, a0, a1);
      sell_st2(ylo + i, a0 + cl * v0, a1 + cl * v1);
      sell_ld2(yhi + i, a0, a1);
      sell_st2(yhi + i, a0 + ch * v0, a1 + ch * v1);
    }
  }
  if (EIG_HAS_TAIL(n)) {
    const int64_t i = n - 1;
    const double v0 = v[i];
    const double r0 = first ? w[i] - alpha * v0 : w[i] - alpha * v0 - beta * vprev[i];
    vprev[i] = r0;
    acc += r0 * r0;
    if (VEC) { ylo[i] += cl * v0; yhi[i] += ch * v0; }
  }
  acc = eig_block_sum(acc, lds);
  if (threadIdx.x == 0) part_out[blockIdx.x] = acc;
}

// beta = sqrt(sum of the partial sums of r.r) (every block); r *= 1 / beta; block 0 stores beta (beta_out may be null)
__global__ __launch_bounds__(256) void k_lanczos_scale(double* __restrict__ r, int64_t n, const double* __restrict__ part,
                                                       int n_part, double* __restrict__ beta_out) {
  __shared__ double lds[4];
  const double beta = sqrt(eig_total_of_partials(part, n_part, lds));
  const double inv = 1.0 / beta;
  if (beta_out && blockIdx.x == 0 && threadIdx.x == 0) *beta_out = beta;
  EIG_PAIR_LOOP(p, n) {
    double a, b;
    sell_ld2(r + 2 * p, a, b);
    sell_st2(r + 2 * p, a * inv, b * inv);
  }
  if (EIG_HAS_TAIL(n)) r[n - 1] *= inv;
}

// ------------------------------------------------------------------------------------------------
// host: extremes of the symmetric tridiagonal T = (alpha[0..m), beta[0..m-1))
// ------------------------------------------------------------------------------------------------
// eigenvalues of T below x (Sturm sequence of the LDL^T pivots; a pivot inside +-pivmin counts as negative)
static int eig_sturm_count(const double* a, const double* b2, int m, double x, double pivmin) {
  int c = 0;
  double q = a[0] - x;
  if (fabs(q) < pivmin) q = -pivmin;
  if (q < 0.0) ++c;
  for (int i = 1; i < m; ++i) {
    q = a[i] - x - b2[i - 1] / q;
    if (fabs(q) < pivmin) q = -pivmin;
    if (q < 0.0) ++c;
  }
  return c;
}

// k-th eigenvalue (ascending, from 0) by bisection of [lo, hi] until no double lies between the ends
static double eig_bisect(const double* a, const double* b2, int m, int k, double lo, double hi, double pivmin) {
  for (int it = 0; it < 2200; ++it) {
    const double mid = lo + 0.5 * (hi - lo);
    if (!(mid > lo && mid < hi)) break;
    if (eig_sturm_count(a, b2, m, mid, pivmin) > k) hi = mid; else lo = mid;
  }
  return lo + 0.5 * (hi - lo);
}

// normalised eigenvector of T to the computed eigenvalue theta: inverse iteration on T - theta I, factored once with
// partial pivoting (pivots below eps |T| are replaced by it), from a fixed pseudo-random start
static void eig_tridiag_vector(const double* a, const double* b, int m, double theta, double tnorm, std::vector<double>& x) {
  x.assign((size_t)m, 1.0);
  if (m == 1) return;
  const double tiny = (tnorm > 0.0 ? tnorm : 1.0) * 2.220446049250313e-16;
  std::vector<double> d((size_t)m), dl((size_t)m - 1), du((size_t)m - 1), du2((size_t)m, 0.0);
  std::vector<char> piv((size_t)m - 1, 0);
  for (int i = 0; i < m; ++i) d[i] = a[i] - theta;
  for (int i = 0; i + 1 < m; ++i) dl[i] = du[i] = b[i];
  for (int i = 0; i + 1 < m; ++i) {
    if (fabs(d[i]) >= fabs(dl[i])) {
      if (fabs(d[i]) < tiny) d[i] = tiny;
      const double f = dl[i] / d[i];
      dl[i] = f;
      d[i + 1] -= f * du[i];
    } else {   // rows i and i + 1 change places
      const double f = d[i] / dl[i];
      d[i] = dl[i];
      dl[i] = f;
      const double t = du[i];
      du[i] = d[i + 1];
      d[i + 1] = t - f * d[i + 1];
      if (i + 2 < m) { du2[i] = du[i + 1]; du[i + 1] = -f * du[i + 1]; }
      piv[i] = 1;
    }
  }
  if (fabs(d[m - 1]) < tiny) d[m - 1] = tiny;
  unsigned long long h = 0x632BE59BD9B4E019ull;
  for (int i = 0; i < m; ++i) {
    h = h * 6364136223846793005ull + 1442695040888963407ull;
    x[i] = 0.5 + (double)(h >> 11) * (1.0 / 9007199254740992.0);   // in [0.5, 1.5)
  }
  for (int it = 0; it < 5; ++it) {
    for (int i = 0; i + 1 < m; ++i) {
      if (!piv[i]) {
        x[i + 1] -= dl[i] * x[i];
      } else {
        const double t = x[i];
        x[i] = x[i + 1];
        x[i + 1] = t - dl[i] * x[i];
      }
    }
    x[m - 1] /= d[m - 1];
    x[m - 2] = (x[m - 2] - du[m - 2] * x[m - 1]) / d[m - 2];
    for (int i = m - 3; i >= 0; --i) x[i] = (x[i] - du[i] * x[i + 1] - du2[i] * x[i + 2]) / d[i];
    double big = 0.0;
    for (int i = 0; i < m; ++i) big = fmax(big, fabs(x[i]));
    if (!(big > 0.0) || !isfinite(big)) { x.assign((size_t)m, 0.0); x[m - 1] = 1.0; return; }   // (not reached with finite T)
    double nrm = 0.0;
    for (int i = 0; i < m; ++i) { x[i] /= big; nrm += x[i] * x[i]; }
    nrm = sqrt(nrm);
    for (int i = 0; i < m; ++i) x[i] /= nrm;
  }
}

// theta_min, theta_max and (when asked) their normalised eigenvectors; false when T holds a non-finite entry.  The work is
// done on T scaled by a power of two to a norm in [1, 2) (exact: neither beta^2 nor the pivot floor meets the ends of the
// exponent range, whatever the units of the operator)
static bool eig_tridiag_extremes(const double* a0, const double* b0, int m, double* th_lo, double* th_hi, std::vector<double>* x_lo,
                                 std::vector<double>* x_hi) {
  double tnorm = 0.0;
  for (int i = 0; i < m; ++i) {
    const double r = (i > 0 ? fabs(b0[i - 1]) : 0.0) + (i + 1 < m ? fabs(b0[i]) : 0.0);
    if (!isfinite(a0[i]) || !isfinite(r) || !isfinite(fabs(a0[i]) + r)) return false;
    tnorm = fmax(tnorm, fabs(a0[i]) + r);
  }
  const int ex = tnorm > 0.0 ? ilogb(tnorm) : 0;
  std::vector<double> as((size_t)m), bs((size_t)(m > 1 ? m - 1 : 1), 0.0);
  for (int i = 0; i < m; ++i) as[i] = ldexp(a0[i], -ex);
  for (int i = 0; i + 1 < m; ++i) bs[i] = ldexp(b0[i], -ex);
  const double* a = as.data();
  const double* b = bs.data();
  tnorm = ldexp(tnorm, -ex);
  double lo = a[0], hi = a[0];
  if (m > 1) {
    double glo = a[0], ghi = a[0];
    for (int i = 0; i < m; ++i) {
      const double r = (i > 0 ? fabs(b[i - 1]) : 0.0) + (i + 1 < m ? fabs(b[i]) : 0.0);
      glo = fmin(glo, a[i] - r);
      ghi = fmax(ghi, a[i] + r);
    }
    std::vector<double> b2((size_t)m - 1);
    for (int i = 0; i + 1 < m; ++i) b2[i] = b[i] * b[i];
    const double pivmin = 1e-290;
    const double pad = 4.0 * 2.220446049250313e-16 * tnorm + pivmin;
    lo = eig_bisect(a, b2.data(), m, 0, glo - pad, ghi + pad, pivmin);
    hi = eig_bisect(a, b2.data(), m, m - 1, glo - pad, ghi + pad, pivmin);
  }
  if (x_lo) eig_tridiag_vector(a, b, m, lo, tnorm, *x_lo);
  if (x_hi) eig_tridiag_vector(a, b, m, hi, tnorm, *x_hi);
  *th_lo = ldexp(lo, ex);
  *th_hi = ldexp(hi, ex);
  return true;
}

int pph_tridiag_extremes(const double* alpha, const double* beta, int m, double* out4) {
  if (!alpha || !out4 || m < 1 || (m > 1 && !beta)) {
    pph_set_error(nullptr, "pph_tridiag_extremes: need alpha[m], beta[m - 1] and out4 with m >= 1");
    return PPH_ERR_INVALID;
  }
  std::vector<double> xl, xh;
  if (!eig_tridiag_extremes(alpha, beta, m, &out4[0], &out4[1], &xl, &xh)) {
    pph_set_error(nullptr, "pph_tridiag_extremes: the tridiagonal matrix holds a value that is not finite");
    return PPH_ERR_INVALID;
  }
  out4[2] = xl[m - 1];
  out4[3] = xh[m - 1];
  return PPH_OK;
}

// ------------------------------------------------------------------------------------------------
// the iteration
// ------------------------------------------------------------------------------------------------
namespace {
struct EigWork {   // everything the call owns: released on every way out
  DevBuf<double> v[3], ab, s, ylo, yhi;
  double* h = nullptr;   // pinned: alpha[max_it] | beta[max_it] | 4 results of the vector pass
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EigWork() {
    for (auto& b : v) b.release();
    ab.release(); s.release(); ylo.release(); yhi.release();
    if (h) (void)hipHostFree(h);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};
}   // namespace

int pph_eig_lanczos(pph_ctx* ctx, const Csr& A, double tol, int max_it, int check_every, double* vec_lo, double* vec_hi,
                    double* out) {
  if (!(tol > 0.0)) tol = 1e-10;
  if (max_it <= 0) max_it = 20000;
  if (check_every <= 0) check_every = 32;
  const int64_t n = A.nrows;
  PPH_REQUIRE(ctx, n >= 1, "extreme eigenvalues of an empty operator");
  const bool vectors = vec_lo || vec_hi;
  PPH_REQUIRE(ctx, !vectors || vec_lo != vec_hi, "vec_lo and vec_hi must be two arrays");
  const int grid = eig_grid(n);
  double* const part_a = ctx->scal.p + PPH_MAX_SCAL + (size_t)EIG_PART_AREA * PPH_PART_STRIDE;   // v.w
  double* const part_v = part_a + PPH_PART_STRIDE;                                                  // r.r

  EigWork W;
  for (auto& b : W.v) PPH_TRY(b.alloc(ctx, (size_t)n));
  PPH_TRY(W.ab.alloc(ctx, 2 * (size_t)max_it + 4));
  PPH_HIP(ctx, hipHostMalloc((void**)&W.h, sizeof(double) * (2 * (size_t)max_it + 4), hipHostMallocDefault));
  PPH_HIP(ctx, hipEventCreate(&W.e0));
  PPH_HIP(ctx, hipEventCreate(&W.e1));
  double* const alpha_d = W.ab.p;
  double* const beta_d = W.ab.p + max_it;
  double* const res_d = W.ab.p + 2 * (size_t)max_it;
  double* const alpha_h = W.h;
  double* const beta_h = W.h + max_it;
  double* const res_h = W.h + 2 * (size_t)max_it;

  la_flush_final(ctx);
  PPH_HIP(ctx, hipEventRecord(W.e0, ctx->stream));

  double *v = nullptr, *vprev = nullptr, *w = nullptr;
  auto start = [&]() {
    v = W.v[0].p; vprev = W.v[1].p; w = W.v[2].p;
    hipLaunchKernelGGL(k_eig_start, dim3(grid), dim3(256), 0, ctx->stream, v, n, part_v);
    hipLaunchKernelGGL(k_lanczos_scale, dim3(grid), dim3(256), 0, ctx->stream, v, n, (const double*)part_v, grid, (double*)nullptr);
  };
  // w = A x and the partial sums of x.w
  auto product = [&](const double* x) {
    la_spmv(ctx, A, x, w);
    hipLaunchKernelGGL(k_lanczos_dot, dim3(grid), dim3(256), 0, ctx->stream, x, (const double*)w, n, part_a);
  };
  auto steps = [&](int j0, int j1, bool vec, int m) {
    for (int j = j0; j < j1; ++j) {
      product(v);
      const double* bp = j > 0 ? beta_d + (j - 1) : (const double*)nullptr;
      if (vec)
        hipLaunchKernelGGL((k_lanczos_update<true>), dim3(grid), dim3(256), 0, ctx->stream, (const double*)w, (const double*)v, vprev,
                           n, (const double*)part_a, grid, bp, alpha_d + j, part_v, W.ylo.p ? W.ylo.p : vec_lo, W.yhi.p ? W.yhi.p : vec_hi,
                           (const double*)(W.s.p + j), (const double*)(W.s.p + m + j));
      else
        hipLaunchKernelGGL((k_lanczos_update<false>), dim3(grid), dim3(256), 0, ctx->stream, (const double*)w, (const double*)v, vprev,
                           n, (const double*)part_a, grid, bp, alpha_d + j, part_v, (double*)nullptr, (double*)nullptr, (const double*)nullptr,
                           (const double*)nullptr);
      hipLaunchKernelGGL(k_lanczos_scale, dim3(grid), dim3(256), 0, ctx->stream, vprev, n, (const double*)part_v, grid, beta_d + j);
      double* t = v; v = vprev; vprev = t;   // (w keeps its buffer: the old v_prev is the new v, the old v the new v_prev)
    }
  };

  double th[2] = {0, 0}, est[2] = {0, 0};
  bool conv[2] = {false, false};
  bool breakdown = false;
  int m = 0, mt = 0;
  std::vector<double> xs[2];   // eigenvectors of T of the two ends
  start();
  while (true) {
    const int m1 = (m + check_every < max_it) ? m + check_every : max_it;
    steps(m, m1, false, 0);
    m = m1;
    PPH_HIP(ctx, hipMemcpyAsync(alpha_h, alpha_d, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(beta_h, beta_d, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // breakdown: the recurrence reached an invariant subspace at step j - T of j + 1 rows is exact
    double scale = isfinite(beta_h[0]) ? beta_h[0] : 0.0;
    mt = m;
    for (int j = 0; j < m; ++j) {
      scale = fmax(scale, fabs(alpha_h[j]));
      if (!isfinite(beta_h[j]) || !(beta_h[j] > EIG_BREAKDOWN * scale)) { mt = j + 1; breakdown = true; break; }
    }
    PPH_REQUIRE(ctx, eig_tridiag_extremes(alpha_h, beta_h, mt, &th[0], &th[1], breakdown ? nullptr : &xs[0], breakdown ? nullptr : &xs[1]),
                "Lanczos: the operator produced values that are not finite (step %d)", mt);
    if (breakdown) {
      est[0] = est[1] = 0.0;
      conv[0] = conv[1] = true;
      break;
    }
    for (int e = 0; e < 2; ++e) {
      est[e] = fabs(beta_h[m - 1] * xs[e][m - 1]);
      if (est[e] <= tol * fabs(th[e])) conv[e] = true;   // (latched: a ghost copy forming at this end later does not undo it)
    }
    if ((conv[0] && conv[1]) || m >= max_it) break;
  }
  for (int i = 0; i < 13; ++i) out[i] = 0.0;
  out[0] = th[0]; out[1] = th[1]; out[2] = (double)m; out[3] = (conv[0] && conv[1]) ? 1.0 : 0.0; out[4] = breakdown ? 1.0 : 0.0;
  out[5] = est[0]; out[6] = est[1]; out[12] = (double)mt;

  if (vectors) {
    // second pass: the same recurrence from the same start (same kernels, same bits), accumulating y = V s for both ends
    if (breakdown) eig_tridiag_extremes(alpha_h, beta_h, mt, &th[0], &th[1], &xs[0], &xs[1]);
    const std::vector<double>&xl = xs[0], &xh = xs[1];
    PPH_TRY(W.s.alloc(ctx, 2 * (size_t)mt));
    if (!vec_lo) PPH_TRY(W.ylo.alloc(ctx, (size_t)n));
    if (!vec_hi) PPH_TRY(W.yhi.alloc(ctx, (size_t)n));
    double* ylo = vec_lo ? vec_lo : W.ylo.p;
    double* yhi = vec_hi ? vec_hi : W.yhi.p;
    // (pageable sources: the copies are staged before hipMemcpyAsync returns)
    PPH_HIP(ctx, hipMemcpyAsync(W.s.p, xl.data(), sizeof(double) * (size_t)mt, hipMemcpyHostToDevice, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(W.s.p + mt, xh.data(), sizeof(double) * (size_t)mt, hipMemcpyHostToDevice, ctx->stream));
    PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    la_set(ctx, ylo, 0.0, n);
    la_set(ctx, yhi, 0.0, n);
    start();
    steps(0, mt, true, mt);
    double* ys[2] = {ylo, yhi};
    for (int e = 0; e < 2; ++e) {
      hipLaunchKernelGGL(k_eig_sumsq, dim3(grid), dim3(256), 0, ctx->stream, (const double*)ys[e], n, part_v);
      hipLaunchKernelGGL(k_lanczos_scale, dim3(grid), dim3(256), 0, ctx->stream, ys[e], n, (const double*)part_v, grid, (double*)nullptr);
      // Rayleigh quotient y.Ay of the normalised vector and || A y - rq y ||: the step's own two kernels on (w, y)
      product(ys[e]);
      hipLaunchKernelGGL((k_lanczos_update<false>), dim3(grid), dim3(256), 0, ctx->stream, (const double*)w, (const double*)ys[e], v,
                         n, (const double*)part_a, grid, (const double*)nullptr, res_d + 2 * e, part_v, (double*)nullptr, (double*)nullptr,
                         (const double*)nullptr, (const double*)nullptr);
      hipLaunchKernelGGL(k_lanczos_scale, dim3(grid), dim3(256), 0, ctx->stream, v, n, (const double*)part_v, grid, res_d + 2 * e + 1);
    }
    PPH_HIP(ctx, hipMemcpyAsync(res_h, res_d, sizeof(double) * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  PPH_HIP(ctx, hipEventRecord(W.e1, ctx->stream));
  PPH_HIP(ctx, hipEventSynchronize(W.e1));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  PPH_HIP(ctx, hipEventElapsedTime(&ms, W.e0, W.e1));
  out[7] = (double)ms;
  if (vectors) { out[8] = res_h[0]; out[9] = res_h[2]; out[10] = res_h[1]; out[11] = res_h[3]; }
  PPH_HIP(ctx, hipGetLastError());
  return PPH_OK;
}

// ------------------------------------------------------------------------------------------------
// K-PCEIG: the extreme eigenvalues of B A (A symmetric positive definite, B a symmetric positive definite preconditioner
// application) by Lanczos for the pencil (A, B^-1): two sequences u_j and v_j = B u_j with u_i . v_j = delta_ij, so that
// T = V^T A V is tridiagonal and carries the spectrum of B A.  B^-1 is never applied.
//
// One step j, besides the product and the preconditioner: k_lanczos_dot (v.w), k_pclanczos_update (alpha_j from the partial
// sums, r = w - alpha_j u - beta_{j-1} u_prev over u_prev), k_lanczos_dot (r.z), k_pclanczos_scale (beta_j = sqrt(r.z),
// u_next = r / beta_j and v_next = z / beta_j in one pass): 16 n + 32 n + 16 n + 32 n = 96 n bytes.  alpha, beta and the raw
// r.z (whose sign tells an indefinite B from a breakdown) travel through device memory, as in the plain iteration.
// The iteration runs on the free rows: the start vector is 0 on the constrained ones, the products keep them 0 (unit rows)
// and pc_operator_apply returns 0 there - the operator the Krylov loops see, whose residuals are 0 on those rows.
// ------------------------------------------------------------------------------------------------
// start vector: the hash of k_eig_start, 0 where a mask is set (rows [0, n0) under m0, rows [n0, n) under m1; null: free)
__global__ __launch_bounds__(256) void k_pceig_start(double* __restrict__ u, int64_t n, const uint8_t* __restrict__ m0,
                                                     const uint8_t* __restrict__ m1, int64_t n0) {
  auto value = [&](int64_t i) {
    const uint8_t* m = i < n0 ? m0 : m1;
    return (m && m[i < n0 ? i : i - n0]) ? 0.0 : eig_hash(i);
  };
  EIG_PAIR_LOOP(p, n) sell_st2(u + 2 * p, value(2 * p), value(2 * p + 1));
  if (EIG_HAS_TAIL(n)) u[n - 1] = value(n - 1);
}

// alpha = sum of k_lanczos_dot's partial sums of v.w (every block, k_reduce_final's order); r = w - alpha u - beta u_prev
// written over u_prev; block 0 stores alpha.  beta_prev null: first step, u_prev is not read.
__global__ __launch_bounds__(256) void k_pclanczos_update(const double* __restrict__ w, const double* __restrict__ u,
                                                          double* __restrict__ uprev, int64_t n,
                                                          const double* __restrict__ part_in, int n_in,
                                                          const double* __restrict__ beta_prev, double* __restrict__ alpha_out) {
  __shared__ double lds[4];
  const double alpha = eig_total_of_partials(part_in, n_in, lds);
  const bool first = beta_prev == nullptr;
  const double beta = first ? 0.0 : *beta_prev;
  if (blockIdx.x == 0 && threadIdx.x == 0) *alpha_out = alpha;
  EIG_PAIR_LOOP(p, n) {
    const int64_t i = 2 * p;
    double w0, w1, u0, u1, q0 = 0.0, q1 = 0.0;
    sell_ld2(w + i, w0, w1);
    sell_ld2(u + i, u0, u1);
    if (!first) sell_ld2(uprev + i, q0, q1);
    const double r0 = first ? w0 - alpha * u0 : w0 - alpha * u0 - beta * q0;
    const double r1 = first ? w1 - alpha * u1 : w1 - alpha * u1 - beta * q1;
    sell_st2(uprev + i, r0, r1);
  }
  if (EIG_HAS_TAIL(n)) {
    const int64_t i = n - 1;
    uprev[i] = first ? w[i] - alpha * u[i] : w[i] - alpha * u[i] - beta * uprev[i];
  }
}

// rz = sum of the partial sums of r.z (every block); beta = sqrt(rz); r *= 1 / beta and z *= 1 / beta in one pass; block 0
// stores beta and the raw rz (either may be null).  A negative rz gives NaNs that nobody reads: the host refuses the run.
__global__ __launch_bounds__(256) void k_pclanczos_scale(double* __restrict__ r, double* __restrict__ z, int64_t n,
                                                         const double* __restrict__ part, int n_part,
                                                         double* __restrict__ beta_out, double* __restrict__ rz_out) {
  __shared__ double lds[4];
  const double rz = eig_total_of_partials(part, n_part, lds);
  const double beta = sqrt(rz);
  const double inv = 1.0 / beta;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (beta_out) *beta_out = beta;
    if (rz_out) *rz_out = rz;
  }
  EIG_PAIR_LOOP(p, n) {
    double a, b;
    sell_ld2(r + 2 * p, a, b);
    sell_st2(r + 2 * p, a * inv, b * inv);
    sell_ld2(z + 2 * p, a, b);
    sell_st2(z + 2 * p, a * inv, b * inv);
  }
  if (EIG_HAS_TAIL(n)) { r[n - 1] *= inv; z[n - 1] *= inv; }
}

namespace {
struct PcEigWork {   // everything the call owns: released on every way out
  DevBuf<double> v[5], ab;
  double* h = nullptr;   // pinned: alpha[max_it] | beta[max_it] | rz[max_it] | u.v of the start
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~PcEigWork() {
    for (auto& b : v) b.release();
    ab.release();
    if (h) (void)hipHostFree(h);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};
}   // namespace

int pph_eig_pclanczos(pph_ctx* ctx, const Csr& A, const PcOperator& P, double tol, int max_it, int check_every, double* out) {
  if (!(tol > 0.0)) tol = 1e-4;
  if (max_it <= 0) max_it = 2000;
  if (check_every <= 0) check_every = 16;
  const int64_t n = A.nrows;
  PPH_REQUIRE(ctx, n >= 1 && n == P.nrows, "preconditioned extremes: operator and preconditioner differ in size");
  const int grid = eig_grid(n);
  double* const part_a = ctx->scal.p + PPH_MAX_SCAL + (size_t)EIG_PART_AREA * PPH_PART_STRIDE;   // v.w
  double* const part_z = part_a + PPH_PART_STRIDE;                                                  // r.z

  PcEigWork W;
  for (auto& b : W.v) PPH_TRY(b.alloc(ctx, (size_t)n));
  const size_t nab = 3 * (size_t)max_it + 1;
  PPH_TRY(W.ab.alloc(ctx, nab));
  PPH_HIP(ctx, hipHostMalloc((void**)&W.h, sizeof(double) * nab, hipHostMallocDefault));
  PPH_HIP(ctx, hipEventCreate(&W.e0));
  PPH_HIP(ctx, hipEventCreate(&W.e1));
  double* const alpha_d = W.ab.p;
  double* const beta_d = W.ab.p + max_it;
  double* const rz_d = W.ab.p + 2 * (size_t)max_it;
  double* const uv_d = W.ab.p + 3 * (size_t)max_it;
  double* const alpha_h = W.h;
  double* const beta_h = W.h + max_it;
  double* const rz_h = W.h + 2 * (size_t)max_it;
  double* const uv_h = W.h + 3 * (size_t)max_it;

  la_flush_final(ctx);
  PPH_HIP(ctx, hipEventRecord(W.e0, ctx->stream));

  double *u = W.v[0].p, *uprev = W.v[1].p, *v = W.v[2].p, *w = W.v[3].p, *z = W.v[4].p;
  // start: u = masked hash, v = B u, both divided by sqrt(u.v)
  const int64_t n0 = P.mask[1] ? n / 2 : n;
  hipLaunchKernelGGL(k_pceig_start, dim3(grid), dim3(256), 0, ctx->stream, u, n, P.mask[0], P.mask[1], n0);
  PPH_TRY(pc_operator_apply(ctx, P, u, v));
  hipLaunchKernelGGL(k_lanczos_dot, dim3(grid), dim3(256), 0, ctx->stream, (const double*)u, (const double*)v, n, part_z);
  hipLaunchKernelGGL(k_pclanczos_scale, dim3(grid), dim3(256), 0, ctx->stream, u, v, n, (const double*)part_z, grid,
                     (double*)nullptr, uv_d);
  PPH_HIP(ctx, hipMemcpyAsync(uv_h, uv_d, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  PPH_REQUIRE(ctx, *uv_h != 0.0, "preconditioned extremes: no free rows (every row of the operator is constrained)");
  // (u.v carries the units of B, not those of B A: the sign rule of the steps has no scale for it, any negative value is one)
  PPH_REQUIRE(ctx, *uv_h > 0.0 && isfinite(*uv_h),
              "preconditioned extremes: the preconditioner is not positive definite on the Krylov space (start: u.Bu = %.3e)", *uv_h);

  double th[2] = {0, 0}, est[2] = {0, 0};
  bool conv[2] = {false, false};
  bool breakdown = false;
  int m = 0, mt = 0;
  std::vector<double> xs[2];   // eigenvectors of T of the two ends
  while (true) {
    const int m1 = (m + check_every < max_it) ? m + check_every : max_it;
    for (int j = m; j < m1; ++j) {
      la_spmv(ctx, A, v, w);
      hipLaunchKernelGGL(k_lanczos_dot, dim3(grid), dim3(256), 0, ctx->stream, (const double*)v, (const double*)w, n, part_a);
      hipLaunchKernelGGL(k_pclanczos_update, dim3(grid), dim3(256), 0, ctx->stream, (const double*)w, (const double*)u, uprev, n,
                         (const double*)part_a, grid, j > 0 ? beta_d + (j - 1) : (const double*)nullptr, alpha_d + j);
      PPH_TRY(pc_operator_apply(ctx, P, uprev, z));
      hipLaunchKernelGGL(k_lanczos_dot, dim3(grid), dim3(256), 0, ctx->stream, (const double*)uprev, (const double*)z, n, part_z);
      hipLaunchKernelGGL(k_pclanczos_scale, dim3(grid), dim3(256), 0, ctx->stream, uprev, z, n, (const double*)part_z, grid,
                         beta_d + j, rz_d + j);
      double* t = u; u = uprev; uprev = t;   // the scaled r is the new u, the old u the new u_prev
      t = v; v = z; z = t;                   // the scaled z is the new v; the old v's buffer receives the next z
    }
    m = m1;
    PPH_HIP(ctx, hipMemcpyAsync(W.h, W.ab.p, sizeof(double) * nab, hipMemcpyDeviceToHost, ctx->stream));
    PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // per step, in order: the sign of r.z (B not positive definite: refused), then the breakdown test of the plain iteration
    double scale = isfinite(beta_h[0]) ? beta_h[0] : 0.0;
    mt = m;
    for (int j = 0; j < m; ++j) {
      scale = fmax(scale, fabs(alpha_h[j]));
      PPH_REQUIRE(ctx, !(rz_h[j] < -EIG_BREAKDOWN * scale * scale),
                  "preconditioned extremes: the preconditioner is not positive definite on the Krylov space (step %d: r.Br = %.3e)",
                  j, rz_h[j]);
      if (!isfinite(beta_h[j]) || !(beta_h[j] > EIG_BREAKDOWN * scale)) { mt = j + 1; breakdown = true; break; }
    }
    PPH_REQUIRE(ctx, eig_tridiag_extremes(alpha_h, beta_h, mt, &th[0], &th[1], breakdown ? nullptr : &xs[0], breakdown ? nullptr : &xs[1]),
                "preconditioned Lanczos: the operator or the preconditioner produced values that are not finite (step %d)", mt);
    if (breakdown) {
      est[0] = est[1] = 0.0;
      conv[0] = conv[1] = true;
      break;
    }
    for (int e = 0; e < 2; ++e) {
      est[e] = fabs(beta_h[m - 1] * xs[e][m - 1]);
      if (est[e] <= tol * fabs(th[e])) conv[e] = true;   // (latched, as in pph_eig_lanczos)
    }
    if ((conv[0] && conv[1]) || m >= max_it) break;
  }
  PPH_HIP(ctx, hipEventRecord(W.e1, ctx->stream));
  PPH_HIP(ctx, hipEventSynchronize(W.e1));
  float ms = 0.f;
  PPH_HIP(ctx, hipEventElapsedTime(&ms, W.e0, W.e1));
  for (int i = 0; i < 10; ++i) out[i] = 0.0;
  out[0] = th[0]; out[1] = th[1]; out[2] = (double)m; out[3] = (conv[0] && conv[1]) ? 1.0 : 0.0; out[4] = breakdown ? 1.0 : 0.0;
  out[5] = est[0]; out[6] = est[1]; out[7] = (double)ms; out[8] = (double)mt; out[9] = P.setup_ms;
  PPH_HIP(ctx, hipGetLastError());
  return PPH_OK;
}
