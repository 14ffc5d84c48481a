// Pathlines and travel times: particles carried by v(x) = scale * u_h(x), u_h a CG-1 vector field of the context's mesh
// (u[node * dim + c], what pph_darcy_velocity_device writes), on all four cell kinds.  Without a reference counterpart (the
// reference draws fd.quiver of the projected velocity, src/perphil/utils/postprocessing.py:34-63, and stops there).
//
// One lane per particle, fp64, classical RK4 with a fixed step dt; location and bases are pph_locate.h's, shared with
// pph_eval.hip.  u_h is continuous, so a path does not depend on which of two neighbouring cells a face point goes to.
//
// A step from x (INSIDE: every coordinate in [0, 1]; NaN is outside; no tolerance):
//   k1 = v(x); |k1|_2 <= min_speed: the particle ends STAGNANT (2)
//   x2 = x + dt/2 k1, k2 = v(x2); x3 = x + dt/2 k2, k3 = v(x3); x4 = x + dt k3, k4 = v(x4);
//   xn = x + dt/6 (k1 + 2 k2 + 2 k3 + k4)
//   x2, x3, x4 and xn all inside: s += |xn - x|_2, x = xn, t += dt, k += 1.
//   Otherwise (as soon as one of them is outside; the later stages are then never needed) the EXIT STEP from x along k1:
//     theta = min_e d_e / |k1_e| over the directions with k1_e != 0, d_e the distance from x_e to the face k1_e points at
//     (the lowest direction wins a tie).  theta <= dt: x += theta k1 with the minimising coordinate set to exactly 0 or 1,
//     t += theta, s += theta |k1|, k += 1, the particle ends EXITED (1) through side 2 e + 1 (x_e = 0) or 2 e + 2 (x_e = 1) -
//     pph_boundary_flux's numbering.  theta > dt: the Euler step x = clamp(x + dt k1, 0, 1), t += dt, k += 1, s += the
//     distance actually moved, and the particle goes on.
//   k == max_steps after a step that did not end the particle: it ends at its STEP LIMIT (0).
// A seed that is not inside ends OUTSIDE (3) with 0 steps and NaN position, time and length.
//
// Keeping waves full.  One launch advances the particles of a live list by at most `chunk` steps each; the outputs (end,
// time, length, steps) hold the state in between.  At the end of its batch every wave appends its survivors to the next
// live list: ballot, prefix count, ONE integer atomic per wave; the two lists are double-buffered and the first launch
// takes the identity list.  The host reads the live count once per launch through the pinned mirror (k_publish's
// protocol) and stops at 0.  The order of a live list varies from run to run; nothing depends on it: every particle is
// independent and, the list append and the status counts apart, there are no atomics - two calls give the same bits, and
// so does any chunk.
//
// Path record (record_every = r > 0): path[j][p][:] = position of particle p after j r steps, j = 0 .. max_steps / r
// ([n_rec][m][dim]: consecutive lanes write consecutive addresses); the buffer is filled with NaN before the first launch,
// so slots a particle never reaches stay NaN.
#include "pph_internal.h"
#include "pph_locate.h"
#include <cmath>

enum { TRACE_S = 48 };   // slots of the host mirror the live count and the four status counts are published to (bit patterns)

struct TraceArgs {
  const int32_t* cells;
  const double* u;
  const double* x0;
  double scale, dt, min_speed;
  EvalGeo g;
  int32_t max_steps, chunk, record_every;
  int64_t m;
  double *end, *time, *length;
  int32_t *steps, *status;
  double* path;                  // NULL: no record
  const int32_t* live_in;        // NULL: the identity list of the first launch, which also checks the seeds
  int32_t n_live;
  int32_t* live_out;
  unsigned long long* n_out;     // length of live_out
  unsigned long long* n_status;  // [4] particles per status
};

template <int DIM>
__device__ static inline bool trace_inside(const double* x) {
  bool in = true;
#pragma unroll
  for (int e = 0; e < DIM; ++e) in = in && (x[e] >= 0.0 && x[e] <= 1.0);
  return in;
}

template <int DIM>
__device__ static inline double trace_norm(const double* v) {
  double q = v[0] * v[0];
#pragma unroll
  for (int e = 1; e < DIM; ++e) q += v[e] * v[e];
  return sqrt(q);
}

// v = scale * u_h(x): the cell's nodes are gathered once and accumulated node by node (nothing but the basis, the running
// sums and one node's components is live at a time)
template <int KIND>
__device__ static inline void trace_velocity(const TraceArgs& a, const double* x, double* v) {
  constexpr int DIM = (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_TRI) ? 2 : 3;
  constexpr bool SIMPLEX = (KIND == PPH_CELL_TRI || KIND == PPH_CELL_TET);
  constexpr int NB = SIMPLEX ? DIM + 1 : (1 << DIM);
  constexpr int CPB = (KIND == PPH_CELL_TRI) ? 2 : (KIND == PPH_CELL_TET) ? 6 : 1;
  double xi[3] = {0.0, 0.0, 0.0};
  int64_t box = 0, stride = 1;
#pragma unroll
  for (int e = 0; e < DIM; ++e) {
    double c;
    xi[e] = box_locate(x[e], a.g.n[e], &c);
    box += stride * (int64_t)c;
    stride *= a.g.n[e];
  }
  double N[NB];
  int sub = 0;
  if constexpr (!SIMPLEX) {
    double w[3][2];
#pragma unroll
    for (int e = 0; e < DIM; ++e) { w[e][0] = 1.0 - xi[e]; w[e][1] = xi[e]; }
#pragma unroll
    for (int b = 0; b < NB; ++b) N[b] = q1_shape<DIM>(w, b);
  } else {
    double lam[DIM + 1], D[DIM + 1][3];
    sub = simplex_locate<KIND>(xi, lam, D);
#pragma unroll
    for (int b = 0; b < NB; ++b) N[b] = lam[b];
  }
  const int32_t* cn = a.cells + (box * CPB + sub) * NB;
#pragma unroll
  for (int c = 0; c < DIM; ++c) v[c] = 0.0;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const double* ub = a.u + (int64_t)cn[b] * DIM;
#pragma unroll
    for (int c = 0; c < DIM; ++c) v[c] += N[b] * ub[c];
  }
#pragma unroll
  for (int c = 0; c < DIM; ++c) v[c] *= a.scale;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_trace(TraceArgs a) {
  constexpr int DIM = (KIND == PPH_CELL_QUAD || KIND == PPH_CELL_TRI) ? 2 : 3;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  const int lane = threadIdx.x & 63;
  const double hdt = 0.5 * a.dt, dt6 = a.dt / 6.0;
  // wave-uniform trip count: every lane of a wave takes part in the ballots of its batch
  const int64_t first = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) - lane;
  for (int64_t base = first; base < a.n_live; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + lane;
    const bool valid = i < a.n_live;
    int st = -2;   // -2: no particle in this lane, -1: still running, >= 0: ended in this launch with that status
    int side = 0;
    int64_t p = 0;
    if (valid) {
      p = a.live_in ? (int64_t)a.live_in[i] : i;
      double x[DIM], t, s;
      int k;
      st = -1;
      if (a.live_in) {
#pragma unroll
        for (int e = 0; e < DIM; ++e) x[e] = a.end[p * DIM + e];
        t = a.time[p]; s = a.length[p]; k = a.steps[p];
      } else {
#pragma unroll
        for (int e = 0; e < DIM; ++e) x[e] = a.x0[p * DIM + e];
        t = 0.0; s = 0.0; k = 0;
        if (!trace_inside<DIM>(x)) {
          st = 3;
#pragma unroll
          for (int e = 0; e < DIM; ++e) x[e] = qnan;
          t = qnan; s = qnan;
        } else if (a.path) {
#pragma unroll
          for (int e = 0; e < DIM; ++e) a.path[p * DIM + e] = x[e];
        }
      }
      for (int it = 0; it < a.chunk && st < 0; ++it) {
        double k1[DIM], kk[DIM], acc[DIM], y[DIM];
        trace_velocity<KIND>(a, x, k1);
        const double sp = trace_norm<DIM>(k1);
        if (sp <= a.min_speed) { st = 2; break; }
#pragma unroll
        for (int e = 0; e < DIM; ++e) y[e] = x[e] + hdt * k1[e];
        bool ok = trace_inside<DIM>(y);
        if (ok) {
          trace_velocity<KIND>(a, y, kk);
#pragma unroll
          for (int e = 0; e < DIM; ++e) { acc[e] = k1[e] + 2.0 * kk[e]; y[e] = x[e] + hdt * kk[e]; }
          ok = trace_inside<DIM>(y);
        }
        if (ok) {
          trace_velocity<KIND>(a, y, kk);
#pragma unroll
          for (int e = 0; e < DIM; ++e) { acc[e] += 2.0 * kk[e]; y[e] = x[e] + a.dt * kk[e]; }
          ok = trace_inside<DIM>(y);
        }
        if (ok) {
          trace_velocity<KIND>(a, y, kk);
#pragma unroll
          for (int e = 0; e < DIM; ++e) { acc[e] += kk[e]; y[e] = x[e] + dt6 * acc[e]; }
          ok = trace_inside<DIM>(y);
        }
        if (ok) {
          double d[DIM];
#pragma unroll
          for (int e = 0; e < DIM; ++e) { d[e] = y[e] - x[e]; x[e] = y[e]; }
          s += trace_norm<DIM>(d);
          t += a.dt;
        } else {
          double theta = __longlong_as_double(0x7ff0000000000000LL);
          int emin = -1;
#pragma unroll
          for (int e = 0; e < DIM; ++e) {
            if (k1[e] != 0.0) {
              const double th = ((k1[e] > 0.0) ? 1.0 - x[e] : x[e]) / fabs(k1[e]);
              if (th < theta) { theta = th; emin = e; }   // (strict: the lowest direction wins a tie)
            }
          }
          if (theta <= a.dt) {
#pragma unroll
            for (int e = 0; e < DIM; ++e) {
              x[e] += theta * k1[e];
              if (e == emin) {
                x[e] = (k1[e] > 0.0) ? 1.0 : 0.0;
                side = 2 * e + ((k1[e] > 0.0) ? 2 : 1);
              }
            }
            t += theta;
            s += theta * sp;
            st = 1;
          } else {
            double d[DIM];
#pragma unroll
            for (int e = 0; e < DIM; ++e) {
              const double xe = fmin(fmax(x[e] + a.dt * k1[e], 0.0), 1.0);
              d[e] = xe - x[e];
              x[e] = xe;
            }
            s += trace_norm<DIM>(d);
            t += a.dt;
          }
        }
        ++k;
        if (a.path && k % a.record_every == 0) {
          double* rec = a.path + ((int64_t)(k / a.record_every) * a.m + p) * DIM;
#pragma unroll
          for (int e = 0; e < DIM; ++e) rec[e] = x[e];
        }
        if (st < 0 && k >= a.max_steps) st = 0;
      }
#pragma unroll
      for (int e = 0; e < DIM; ++e) a.end[p * DIM + e] = x[e];
      a.time[p] = t; a.length[p] = s; a.steps[p] = k;
      if (st >= 0) a.status[p] = st | (side << 8);
    }
    // survivors -> next live list: one atomic per wave
    const unsigned long long alive = __ballot(st == -1);
    const int leader = __ffsll((long long)__ballot(1)) - 1;
    if (alive) {
      unsigned long long at = 0;
      if (lane == leader) at = atomicAdd(a.n_out, (unsigned long long)__popcll(alive));
      at = __shfl(at, leader, 64);
      if (st == -1) a.live_out[at + __popcll(alive & ((1ull << lane) - 1ull))] = (int32_t)p;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned long long ended = __ballot(st == q);
      if (ended && lane == leader) atomicAdd(a.n_status + q, (unsigned long long)__popcll(ended));
    }
  }
}

// live count of the list just written and the status counts -> host mirror, the count of the list just read -> 0 (it is
// the list after next's), then the sequence word: k_publish's protocol on the call's own counters
__global__ __launch_bounds__(64) void k_trace_publish(unsigned long long* __restrict__ cnt, int written,
                                                      unsigned long long* __restrict__ hdst,
                                                      unsigned long long* __restrict__ hseq, unsigned long long* ctr) {
  if (threadIdx.x == 0) hdst[0] = cnt[written];
  if (threadIdx.x >= 1 && threadIdx.x < 5) hdst[threadIdx.x] = cnt[1 + threadIdx.x];
  if (threadIdx.x == 5) cnt[written ^ 1] = 0;
  __threadfence_system();
  if (threadIdx.x == 0) {
    const unsigned long long seq = *ctr + 1;
    *ctr = seq;
    __hip_atomic_store(hseq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// device memory of one call: released by the entry point whichever way the call ends
struct TraceBufs {
  DevBuf<int32_t> live[2], steps, status;
  DevBuf<unsigned long long> cnt;   // [0], [1]: lengths of the two live lists; [2..5]: particles per status
  DevBuf<double> u, x0, end, time, length, path;   // (host variant only)
  void release() {
    live[0].release(); live[1].release(); steps.release(); status.release(); cnt.release();
    u.release(); x0.release(); end.release(); time.release(); length.release(); path.release();
  }
};

static int64_t trace_records(int32_t max_steps, int32_t record_every) {
  return record_every > 0 ? (int64_t)(max_steps / record_every) + 1 : 0;
}

static int trace_check(pph_ctx* ctx, const char* who, const void* u, double scale, const void* x0, int64_t m, double dt,
                       int32_t max_steps, double min_speed, int32_t chunk, int32_t record_every, const void* end,
                       const void* time, const void* length, const void* steps, const void* status, const int64_t* counts) {
  PPH_REQUIRE(ctx, ctx->mesh_ok, "%s before pph_mesh_build", who);
  PPH_REQUIRE(ctx, ctx->world == 1, "pathlines are implemented for single-context meshes");
  PPH_REQUIRE(ctx, ctx->mesh.degree == 1, "%s: the traced field lives on the CG-1 vector space (this context holds a degree-%d mesh)",
              who, ctx->mesh.degree);
  PPH_REQUIRE(ctx, std::isfinite(dt) && dt > 0.0, "%s: dt must be finite and positive", who);
  PPH_REQUIRE(ctx, std::isfinite(scale) && scale != 0.0, "%s: scale must be finite and non-zero", who);
  PPH_REQUIRE(ctx, max_steps >= 1, "%s: max_steps must be at least 1, got %d", who, (int)max_steps);
  PPH_REQUIRE(ctx, chunk >= 1, "%s: chunk must be at least 1, got %d", who, (int)chunk);
  PPH_REQUIRE(ctx, record_every >= 0, "%s: record_every must not be negative, got %d", who, (int)record_every);
  PPH_REQUIRE(ctx, min_speed >= 0.0, "%s: min_speed must not be negative or NaN", who);
  PPH_REQUIRE(ctx, m >= 0 && m <= (int64_t)INT32_MAX, "%s: the number of particles must be in [0, 2^31 - 1], got %lld", who,
              (long long)m);
  PPH_REQUIRE(ctx, u && counts && (m == 0 || (x0 && end && time && length && steps && status)), "%s: NULL buffer", who);
  return PPH_OK;
}

template <int KIND>
static void trace_launch(pph_ctx* ctx, int grid, const TraceArgs& a) {
  hipLaunchKernelGGL((k_trace<KIND>), dim3(grid), dim3(256), 0, ctx->stream, a);
}

// device arrays in, device arrays out; returns after the stream has finished with them (the last live count is read)
static int trace_run(pph_ctx* ctx, TraceBufs& b, const double* u, double scale, const double* x0, int64_t m, double dt,
                     int32_t max_steps, double min_speed, int32_t chunk, int32_t record_every, double* end, double* time,
                     double* length, int32_t* steps, int32_t* status, double* path, int64_t* counts) {
  const MeshData& ms = ctx->mesh;
  for (int q = 0; q < 4; ++q) counts[q] = 0;
  if (m == 0) return PPH_OK;
  PPH_TRY(b.live[0].alloc(ctx, (size_t)m));
  PPH_TRY(b.live[1].alloc(ctx, (size_t)m));
  PPH_TRY(b.cnt.alloc(ctx, 6));
  PPH_HIP(ctx, hipMemsetAsync(b.cnt.p, 0, 6 * sizeof(unsigned long long), ctx->stream));
  TraceArgs a;
  a.cells = ms.cells.p; a.u = u; a.x0 = x0;
  a.scale = scale; a.dt = dt; a.min_speed = min_speed;
  a.g.n[0] = ms.nx; a.g.n[1] = ms.ny; a.g.n[2] = (ms.dim == 3) ? ms.nzl : 1;
  a.max_steps = max_steps; a.chunk = chunk; a.record_every = record_every;
  a.m = m;
  a.end = end; a.time = time; a.length = length; a.steps = steps; a.status = status;
  a.path = (record_every > 0) ? path : nullptr;
  a.n_status = b.cnt.p + 2;
  if (a.path)   // slots a particle never reaches hold NaN
    la_set(ctx, path, __builtin_nan(""), trace_records(max_steps, record_every) * m * ms.dim);
  unsigned long long* const hmirror = reinterpret_cast<unsigned long long*>(ctx->h_scal + TRACE_S);
  unsigned long long* const hmirror_dev = reinterpret_cast<unsigned long long*>(ctx->h_scal_dev + TRACE_S);
  int64_t n_live = m;
  for (int launch = 0; n_live > 0; ++launch) {
    const int in = launch & 1, out = in ^ 1;
    a.live_in = launch ? b.live[in].p : nullptr;
    a.n_live = (int32_t)n_live;
    a.live_out = b.live[out].p;
    a.n_out = b.cnt.p + out;
    const int64_t nb = ceil_div64(n_live, 256);
    const int grid = (int)(nb < 8192 ? nb : 8192);
    if (ms.kind == PPH_CELL_QUAD) trace_launch<PPH_CELL_QUAD>(ctx, grid, a);
    else if (ms.kind == PPH_CELL_TRI) trace_launch<PPH_CELL_TRI>(ctx, grid, a);
    else if (ms.kind == PPH_CELL_HEX) trace_launch<PPH_CELL_HEX>(ctx, grid, a);
    else trace_launch<PPH_CELL_TET>(ctx, grid, a);
    PPH_HIP(ctx, hipGetLastError());
    ++ctx->pub_seq;
    hipLaunchKernelGGL(k_trace_publish, dim3(1), dim3(64), 0, ctx->stream, b.cnt.p, out, hmirror_dev, ctx->h_seq_dev,
                       ctx->pub_ctr.p);
    PPH_HIP(ctx, hipGetLastError());
    if (ctx->fetch_spin) PPH_TRY(la_wait_published(ctx));
    else PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    n_live = (int64_t)hmirror[0];
    PPH_REQUIRE(ctx, n_live >= 0 && n_live <= m, "pathlines: live count %lld out of range", (long long)n_live);
  }
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int q = 0; q < 4; ++q) counts[q] = (int64_t)hmirror[1 + q];
  return PPH_OK;
}

static int trace_host(pph_ctx* ctx, TraceBufs& b, const double* u_host, double scale, const double* x0_host, int64_t m, double dt,
                      int32_t max_steps, double min_speed, int32_t chunk, int32_t record_every, double* end_host,
                      double* time_host, double* length_host, int32_t* steps_host, int32_t* status_host, double* path_host,
                      int64_t* counts) {
  const MeshData& ms = ctx->mesh;
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nu = (size_t)ms.n * ms.dim, nx = (size_t)m * ms.dim;
  const size_t np = (record_every > 0 && path_host) ? (size_t)trace_records(max_steps, record_every) * nx : 0;
  PPH_TRY(b.u.alloc(ctx, nu));
  PPH_HIP(ctx, hipMemcpyAsync(b.u.p, u_host, sizeof(double) * nu, hipMemcpyHostToDevice, ctx->stream));
  if (m > 0) {
    PPH_TRY(b.x0.alloc(ctx, nx));
    PPH_TRY(b.end.alloc(ctx, nx));
    PPH_TRY(b.time.alloc(ctx, (size_t)m));
    PPH_TRY(b.length.alloc(ctx, (size_t)m));
    PPH_TRY(b.steps.alloc(ctx, (size_t)m));
    PPH_TRY(b.status.alloc(ctx, (size_t)m));
    if (np) PPH_TRY(b.path.alloc(ctx, np));
    PPH_HIP(ctx, hipMemcpyAsync(b.x0.p, x0_host, sizeof(double) * nx, hipMemcpyHostToDevice, ctx->stream));
  }
  PPH_TRY(trace_run(ctx, b, b.u.p, scale, b.x0.p, m, dt, max_steps, min_speed, chunk, record_every, b.end.p, b.time.p,
                    b.length.p, b.steps.p, b.status.p, np ? b.path.p : nullptr, counts));
  if (m > 0) {
    PPH_HIP(ctx, hipMemcpyAsync(end_host, b.end.p, sizeof(double) * nx, hipMemcpyDeviceToHost, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(time_host, b.time.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(length_host, b.length.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(steps_host, b.steps.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    PPH_HIP(ctx, hipMemcpyAsync(status_host, b.status.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    if (np) PPH_HIP(ctx, hipMemcpyAsync(path_host, b.path.p, sizeof(double) * np, hipMemcpyDeviceToHost, ctx->stream));
  }
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PPH_OK;
}

extern "C" int pph_trace_pathlines(pph_ctx* ctx, const double* u_host, double scale, const double* x0_host, int64_t m, double dt,
                                   int32_t max_steps, double min_speed, int32_t chunk, int32_t record_every,
                                   double* end_host, double* time_host, double* length_host, int32_t* steps_host,
                                   int32_t* status_host, double* path_host, int64_t* counts) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(trace_check(ctx, "pph_trace_pathlines", u_host, scale, x0_host, m, dt, max_steps, min_speed, chunk, record_every,
                      end_host, time_host, length_host, steps_host, status_host, counts));
  TraceBufs b;
  const int st = trace_host(ctx, b, u_host, scale, x0_host, m, dt, max_steps, min_speed, chunk, record_every, end_host,
                            time_host, length_host, steps_host, status_host, path_host, counts);
  b.release();
  return st;
}

extern "C" int pph_trace_pathlines_device(pph_ctx* ctx, const double* u_dev, double scale, const double* x0_dev, int64_t m,
                                          double dt, int32_t max_steps, double min_speed, int32_t chunk, int32_t record_every,
                                          double* end_dev, double* time_dev, double* length_dev, int32_t* steps_dev,
                                          int32_t* status_dev, double* path_dev, int64_t* counts) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_TRY(trace_check(ctx, "pph_trace_pathlines_device", u_dev, scale, x0_dev, m, dt, max_steps, min_speed, chunk, record_every,
                      end_dev, time_dev, length_dev, steps_dev, status_dev, counts));
  TraceBufs b;
  int st = hipSetDevice(ctx->device) == hipSuccess ? PPH_OK : PPH_ERR_HIP;
  if (st == PPH_OK)
    st = trace_run(ctx, b, u_dev, scale, x0_dev, m, dt, max_steps, min_speed, chunk, record_every, end_dev, time_dev,
                   length_dev, steps_dev, status_dev, path_dev, counts);
  b.release();
  return st;
}
