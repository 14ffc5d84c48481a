// Host-side Krylov / preconditioner / Picard drivers over the device kernels of pph_la.hip.
//
// Replaces KSPSolve (GMRES(30) / CG), PCApply (none, jacobi, fieldsplit multiplicative) and the
// SNES(ksponly) wrapper that reference src/perphil/solvers/solver.py:67-74 drives through
// LinearVariationalSolver; the Picard loop is the block iteration stated by dpp_delayed_form
// (reference src/perphil/forms/dpp.py:196-203).  PETSc semantics kept: left preconditioning,
// convergence test on the preconditioned residual, ||r|| <= max(rtol*||P^-1 b||, atol), restart 30,
// classical Gram-Schmidt without refinement, zero initial guess for KSP solves.
#include "pph_internal.h"
#include <chrono>
#include <cmath>
#include <functional>

// slots in ctx->scal used by the drivers
enum { S_A = 0, S_B = 2, S_BAD = 3, S_C = 4, S_INNER = 8, S_COARSE = 16, S_MDOT = 64 };   // S_BAD: breakdowns counted on the device (launch-only sweeps)

// work vector ids
enum {
  W_R = 0, W_Z, W_P, W_Q, W_T,          // outer CG
  W_IR, W_IZ, W_IP, W_IQ,               // inner CG (block solves)
  W_GV, W_GW, W_GT,                     // GMRES basis / work
  W_IGV, W_IGW, W_IGT, W_IGR,           // inner GMRES (block solves): basis / work / residual of a warm start
  W_FS1, W_FS2,                         // field-split temporaries
  W_DINV_M, W_DINV_1, W_DINV_2, W_BINV, // preconditioner data
  W_DU, W_PB, W_T12, W_TN, W_RHS1, W_R1, W_R2,  // Picard: correction, block rhs, coupling terms, block residuals
  W_COUNT
};

static int work(pph_ctx* ctx, int id, size_t n, double** out) {
  if ((int)ctx->work.size() < W_COUNT) ctx->work.resize(W_COUNT);
  DevBuf<double>& b = ctx->work[id];
  if (b.n < n) {
    b.release();
    PPH_TRY(b.alloc(ctx, n));
  }
  *out = b.p;
  return PPH_OK;
}

typedef std::function<void(const double*, double*)> ApplyFn;

struct KspOut {
  int its = 0;
  double res = 0.0;
  bool converged = false;
  bool breakdown = false;
  double bnorm = 0.0;  // ||P^-1 b|| the tolerance was relative to
};

// which: 0 A11, 1 A22, 2 A12, 3 A21.  The product runs on the stencil-ELL copy when the blocks have one
static Csr block_csr(pph_ctx* ctx, int which) {
  Csr A;
  const double* vals[4] = {ctx->A11.p, ctx->A22.p, ctx->A12.p, ctx->A21p()};
  const Sell* ells[4] = {&ctx->S11, &ctx->S22, &ctx->S12, &ctx->S21};
  A.rowptr = ctx->mesh.rowptr.p; A.col = ctx->mesh.col.p; A.val = ctx->csr_ok ? vals[which] : nullptr;
  A.nrows = ctx->n; A.nnz = ctx->nnzb;
  if (ctx->ell_ok && ctx->op_format == 1) A.ell = *ells[which];
  A.max_row = ctx->mesh.max_row;
  A.geom = (ctx->world > 1) ? &ctx->mesh : nullptr;
  A.lanes = pph_pick_lanes(ctx, A.nnz, A.nrows);
  return A;
}

static Csr mono_csr(pph_ctx* ctx) {
  Csr A;
  A.rowptr = ctx->mrowptr.p; A.col = ctx->mcol.p; A.val = ctx->mval.p; A.nrows = 2 * ctx->n; A.nnz = 4 * ctx->nnzb;
  A.max_row = 2 * ctx->mesh.max_row;
  A.geom = (ctx->world > 1) ? &ctx->mesh : nullptr;
  A.lanes = pph_pick_lanes(ctx, A.nnz, A.nrows);
  return A;
}

// ------------------------------------------------------------------------------------------------
// preconditioned CG that tests the UNPRECONDITIONED residual ||r||_2 (KSP_NORM_UNPRECONDITIONED): the
// recurrence residual is known before the preconditioner is applied, so a solve of k iterations costs k
// preconditioner applications instead of k + 1 and a warm start that already meets the tolerance costs
// none.  Tolerance: max(rtol * ||b||_2, atol, reduction * ||r_0||_2).  `bnorm_hint` is ||b||_2 of an
// earlier, nearby system (see cg_solve).
// ------------------------------------------------------------------------------------------------
// by-products the fused multigrid cycle offers to the CG around it (mg_pre_smoother / pph_internal.h)
struct MgPre {
  bool on = false;
  const double* dinv = nullptr;   // z0 = dinv .* r * w is the cycle's first kernel: the CG update writes it instead
  const double* w = nullptr;      // (device)
  int tag = 0;                    // identifies the preconditioner (block, smoothing steps) in the graph cache
  bool launch_only = false;       // the cycle enqueues kernels only (no host decision inside): capturable
};

// what the unpreconditioned-norm CG of one block remembers from solve to solve within a pph_solve_device call: its updates
// write the next cycle's first guess only where a cycle is expected to read it (option "presmooth_lazy")
struct CgMemo {
  double rho = -1.0;   // most recent observed contraction res_k / res_{k-1} (-1: none yet)
  int its = -1;        // iterations of the block's previous solve (-1: none yet)
};

static int cg_solve_natural(pph_ctx* ctx, const Csr& A, const double* b, double* x, const double* dinv, const ApplyFn& pc,
                            double rtol, double atol, int max_it, bool warm, double* r, double* z, double* p, double* q,
                            int slot, KspOut* out, double* hist, int hist_cap, double bnorm_hint, double reduction,
                            const double* r_init, const MgPre& pre, double rnorm_hint = -1.0, bool first_x0_ready = false,
                            CgMemo* memo = nullptr, bool x_is_zero = false) {
  const int64_t n = A.nrows;
  const Seg sg = pph_owned_seg(A.geom, n);
  auto apply_pc = [&](const double* in, double* o) {
    if (dinv) la_pointwise_mult(ctx, o, dinv, in, n);
    else if (pc) pc(in, o);
    else la_copy(ctx, o, in, n);
  };
  double bnorm = -1.0;
  if (warm) {
    if (bnorm_hint > 0.0) {
      bnorm = bnorm_hint;
    } else {
      la_mdot_seg(ctx, b, 0, 1, b, sg, slot);
      PPH_TRY(la_fetch(ctx, slot, 1));
      bnorm = std::sqrt(ctx->h_scal[slot]);
    }
    if (r_init) { if (r_init != r) la_copy(ctx, r, r_init, n); }
    else la_spmv_resid(ctx, A, x, b, r);
  } else {
    if (!x_is_zero) la_set(ctx, x, 0.0, n);
    la_copy(ctx, r, b, n);
  }
  double res;
  if (rnorm_hint >= 0.0 && warm && r_init) {
    res = rnorm_hint;   // the caller knows ||r_init|| (Picard bookkeeping): no reduction, no host round trip
  } else {
    la_mdot_seg(ctx, r, 0, 1, r, sg, slot);
    PPH_TRY(la_fetch(ctx, slot, 1));
    res = std::sqrt(ctx->h_scal[slot]);
  }
  if (bnorm < 0.0) bnorm = res;
  const double tol = std::fmax(std::fmax(rtol * bnorm, atol), reduction > 0.0 ? reduction * res : 0.0);
  out->its = 0; out->res = res; out->converged = false; out->breakdown = false; out->bnorm = bnorm;
  if (hist && hist_cap > 0) hist[0] = res;
  if (!(res == res)) { out->breakdown = true; return PPH_OK; }
  if (res <= tol) { out->converged = true; return PPH_OK; }
  if (la_device_scalars(ctx)) {
    // alpha and beta live in ctx->scal: the host sees p.Ap (breakdown test) and r.r (convergence test) once per
    // iteration, in one copy
    const int sPQ = slot, sRR = slot + 1, sRZn = slot + 2, sRZc = slot + 3;   // p.Ap, r.r, r.z (new), r.z (current)
    // Slabs: ONE all-reduce behind the product instead of one for p.Ap and one for r.r (`merge_allreduce`, stencil-ELL
    // operators).  The product also sums r.Ap and Ap.Ap (mode 7); { p.Ap, r.Ap, Ap.Ap, local r.r of the PREVIOUS update }
    // sit in four consecutive slots and are summed over the ranks together; the host forms the new
    // r.r = r.r_prev - 2 alpha r.Ap + alpha^2 Ap.Ap - one step of the recurrence from a true value, no accumulation of
    // rounding - so an iteration costs two scalar all-reduces (r.z; this one) instead of three.
    const int sE = slot + 4;   // sE .. sE + 2 = p.Ap, r.Ap, Ap.Ap ; sE + 3 = r.r of the previous update
    const bool merged = ctx->merge_allreduce && ctx->world > 1 && !ctx->comm_suspended && A.ell.val != nullptr;
    // z = M^-1 r and r.z -> scal[slot_rz]; a fused multigrid cycle delivers the dot product from its last kernel
    auto pc_and_rz = [&](double* zz, int slot_rz, bool x0_ready) {
      if (pre.on) { ctx->mg_dot_slot = slot_rz; ctx->mg_dot_seg = sg; ctx->mg_x0_ready = x0_ready; }
      apply_pc(r, zz);
      const bool delivered = ctx->mg_dot_slot == -2;
      ctx->mg_dot_slot = -1;
      ctx->mg_x0_ready = false;
      if (!delivered) la_mdot_seg(ctx, r, 0, 1, zz, sg, slot_rz);
    };
    // the two halves of an iteration around the host's convergence test.  `rotate`: r.z (current) := r.z (new) rides
    // on the final reduction of p.Ap - after the direction update read both, before the CG update reads the current one
    bool published = false;   // (the publication of p.Ap and r.r rode on the update's final reduction)
    bool z_ready = false;     // the last update wrote the next cycle's pre-smoothed first guess into z
    auto half_product = [&](bool rotate, bool publish, bool want_z0) -> int {
      published = false;
      z_ready = want_z0;
      if (merged) {
        la_spmv_dot3(ctx, A, p, r, q, sE, rotate ? sRZn : -1, sRZc);
        PPH_TRY(la_reduce_device(ctx, sE, 4));
        la_cg_update_dev(ctx, x, r, p, q, sRZc, sE, n, sE + 3, sg, want_z0 ? z : nullptr, pre.dinv, pre.w);   // (its r.r: local, summed with the next product's)
        return PPH_OK;
      }
      la_spmv_dot(ctx, A, p, q, sPQ, rotate ? sRZn : -1, sRZc, true);   // (its final reduction: inside the update kernel)
      PPH_TRY(la_reduce_device(ctx, sPQ, 1));
      // x += alpha p ; r -= alpha q ; r.r (and the next cycle's pre-smoothed first guess into z)
      published = la_cg_update_dev(ctx, x, r, p, q, sRZc, sPQ, n, sRR, sg, want_z0 ? z : nullptr, pre.dinv, pre.w, -1,
                                   publish ? sPQ : -1, publish ? 2 : 0);
      PPH_TRY(la_reduce_device(ctx, sRR, 1));
      return PPH_OK;
    };
    auto half_direction = [&]() -> int {
      ctx->defer_next_final = true;    // (r.z of the cycle's last kernel: summed inside the direction update)
      if (pre.on && !z_ready) ctx->n_presmooth_late++;   // (the update before was predicted to be the last: k_cheb_init, same bits)
      pc_and_rz(z, sRZn, z_ready);
      ctx->defer_next_final = false;
      PPH_TRY(la_reduce_device(ctx, sRZn, 1));
      la_p_update_dev(ctx, p, z, sRZn, sRZc, n);                          // p = z + (r.z_new / r.z) p
      return PPH_OK;
    };
    pc_and_rz(p, sRZc, first_x0_ready && pre.on);     // first direction p = z_0: written in place (pre-smoothed by the caller?)
    PPH_TRY(la_reduce_device(ctx, sRZc, 1));
    // Iterations after the first are one hipGraph each (direction half, product half, publication of p.Ap and r.r):
    // on small meshes the kernels are shorter than the 3.5 us the host needs to enqueue one, so an eager iteration
    // is host-bound; the captured body replays in one call.  Single context, fused multigrid cycle only.
    GraphKey gk;
    // (measured: a replay starts 38 us after the host's decision, an eager launch 17 us - the replay pays off only
    // where the iteration's kernels are shorter than the host's launch rate.  With the fused cycle and its on-chip tail
    // that is no longer the case at any size measured: 32^3 equal, 64^3 3.45 ms replayed vs 3.15 ms eager, 96^3 equal -
    // graph_cg_max_rows defaults to 0 (off); use_graphs 2: always)
    const bool graphable = ctx->use_graphs && (ctx->use_graphs == 2 || n <= ctx->graph_cg_max_rows) && pre.on && pre.launch_only &&
                           ctx->world == 1 && !ctx->time_spmv && ctx->fetch_spin;
    if (graphable) {
      gk.p[0] = A.ell.val ? (const void*)A.ell.val : (const void*)A.val; gk.p[1] = x; gk.p[2] = r; gk.p[3] = z; gk.p[4] = p;
      gk.p[5] = q; gk.p[6] = pre.dinv; gk.p[7] = pre.w;
      gk.n = n; gk.slot = slot; gk.epoch = ctx->mg_epoch; gk.tag = pre.tag;
    }
    // An update writes z0 = dinv0 .* r * w0 for the cycle of the NEXT iteration - two of its eight vector passes, for
    // nothing when the solve ends with this update.  The host knows `res` and `tol` before it launches the update: the update
    // is taken for the last one when the block's most recent contraction would carry `res` below `tol` (presmooth_lazy 2:
    // when the block's previous solve ended at this iteration), and then passes no z0; if the solve goes on after all, the
    // cycle forms its first guess itself (k_cheb_init: the same expression in the same order, the same bits; three vector
    // passes where the update would have spent two).  At most two such guesses per solve - the first rests on the block's
    // previous solve, the second on this solve's own first contraction; a solve that drifts pays two late starts, not one
    // per iteration.  The numbers are equal on all ranks.  A replayed body has fixed arguments: no skip there.
    const bool lazy = ctx->presmooth_lazy && pre.on && memo && !graphable;
    int guesses = 0;
    auto want_z0 = [&](int k) -> bool {   // for the update of iteration k (0-based)
      if (!lazy) return pre.on;
      bool last = k + 1 >= max_it;
      if (!last && guesses < 2) {
        last = (ctx->presmooth_lazy == 2) ? (memo->its == k + 1) : (memo->rho >= 0.0 && res * memo->rho <= tol);
        guesses += last ? 1 : 0;
      }
      if (last) ctx->n_presmooth_skipped++;
      return !last;
    };
    int its = 0;
    double rr_prev = res * res;   // (merged all-reduce) r.r the recurrence starts from: host-known before the first update
    while (its < max_it) {
      const double res_before = res;
      if (its == 0) {
        PPH_TRY(half_product(false, true, want_z0(0)));
        if (merged) PPH_TRY(la_fetch_raw(ctx, sRZc, 5));   // r.z (current), p.Ap, r.Ap, Ap.Ap, r.r of the previous update
        else if (published) PPH_TRY(la_wait_published(ctx));
        else PPH_TRY(la_fetch_raw(ctx, sPQ, 2));
      } else {
        auto body = [&]() -> int {
          PPH_TRY(half_direction());
          PPH_TRY(half_product(true, true, want_z0(its)));
          if (merged) la_publish(ctx, sRZc, 5);
          else if (!published) la_publish(ctx, sPQ, 2);
          return PPH_OK;
        };
        if (graphable) PPH_TRY(la_run_graph(ctx, gk, body));
        else PPH_TRY(body());
        PPH_TRY(la_wait_published(ctx));
        if (ctx->comm_status != PPH_OK) { ctx->err = ctx->comm_error; return ctx->comm_status; }
      }
      if (merged) {
        if (its > 0) rr_prev = ctx->h_scal[sE + 3];   // the true r.r of the previous update, summed with this product's sums
        const double pqe = ctx->h_scal[sE], rq = ctx->h_scal[sE + 1], qq = ctx->h_scal[sE + 2];
        const double alpha = ctx->h_scal[sRZc] / pqe;
        const double rr = rr_prev - 2.0 * alpha * rq + alpha * alpha * qq;
        ctx->h_scal[sPQ] = pqe;
        ctx->h_scal[sRR] = (rr > 0.0 || rr != rr) ? rr : 0.0;   // (a NaN stays one: breakdown below)
      }
      const double pq = ctx->h_scal[sPQ];
      res = std::sqrt(ctx->h_scal[sRR]);
      ++its;
      if (memo && res_before > 0.0 && res == res) memo->rho = res / res_before;
      if (hist && its < hist_cap) hist[its] = res;
      if (!(pq > 0.0) || !(res == res)) { out->breakdown = true; break; }
      if (res <= tol) { out->converged = true; break; }
    }
    if (z_ready) ctx->n_presmooth_unused++;   // (the last update's z0: no cycle follows)
    if (memo) memo->its = its;
    out->its = its;
    out->res = res;
    return PPH_OK;
  }
  apply_pc(r, z);
  la_mdot_seg(ctx, r, 0, 1, z, sg, slot);
  PPH_TRY(la_fetch(ctx, slot, 1));
  double rz = ctx->h_scal[slot];
  la_copy(ctx, p, z, n);
  int its = 0;
  while (its < max_it) {
    la_spmv_dot(ctx, A, p, q, slot);
    PPH_TRY(la_fetch(ctx, slot, 1));
    const double pq = ctx->h_scal[slot];
    if (!(pq > 0.0) || !(rz == rz)) { out->breakdown = true; break; }
    const double alpha = rz / pq;
    la_cg_update(ctx, x, r, nullptr, p, q, nullptr, alpha, n, slot, sg);   // x += alpha p ; r -= alpha q ; r.r
    PPH_TRY(la_fetch(ctx, slot, 1));
    res = std::sqrt(ctx->h_scal[slot]);
    ++its;
    if (hist && its < hist_cap) hist[its] = res;
    if (!(res == res)) { out->breakdown = true; break; }
    if (res <= tol) { out->converged = true; break; }
    apply_pc(r, z);
    la_mdot_seg(ctx, r, 0, 1, z, sg, slot);
    PPH_TRY(la_fetch(ctx, slot, 1));
    const double rz_new = ctx->h_scal[slot];
    la_axpby(ctx, p, 1.0, z, rz_new / rz, n);
    rz = rz_new;
  }
  out->its = its;
  out->res = res;
  return PPH_OK;
}

// ------------------------------------------------------------------------------------------------
// preconditioned CG without a convergence test (PETSc: ksp_norm_type none + ksp_max_it): exactly `its` iterations,
// every scalar stays on the device, NO host decision inside - a block solve is a pure launch sequence, so a whole
// Picard sweep can be enqueued (and replayed from a graph) without the GPU ever waiting for the host.  No
// preconditioner application after the last update.  Needs the device-scalar branch (la_device_scalars).
// ------------------------------------------------------------------------------------------------
static int cg_solve_fixed(pph_ctx* ctx, const Csr& A, const double* b, double* x, const double* dinv, const ApplyFn& pc,
                          int its, bool warm, double* r, double* z, double* p, double* q, int slot, KspOut* out,
                          const double* r_init, const MgPre& pre, bool first_x0_ready = false, bool x_is_zero = false) {
  const int64_t n = A.nrows;
  const Seg sg = pph_owned_seg(A.geom, n);
  auto apply_pc = [&](const double* in, double* o) {
    if (dinv) la_pointwise_mult(ctx, o, dinv, in, n);
    else if (pc) pc(in, o);
    else la_copy(ctx, o, in, n);
  };
  if (warm) {
    if (r_init) { if (r_init != r) la_copy(ctx, r, r_init, n); }
    else la_spmv_resid(ctx, A, x, b, r);
  } else {
    if (!x_is_zero) la_set(ctx, x, 0.0, n);
    la_copy(ctx, r, b, n);
  }
  const int sPQ = slot, sRR = slot + 1, sRZn = slot + 2, sRZc = slot + 3;
  auto pc_and_rz = [&](double* zz, int slot_rz, bool x0_ready) {
    if (pre.on) { ctx->mg_dot_slot = slot_rz; ctx->mg_dot_seg = sg; ctx->mg_x0_ready = x0_ready; }
    apply_pc(r, zz);
    const bool delivered = ctx->mg_dot_slot == -2;
    ctx->mg_dot_slot = -1;
    ctx->mg_x0_ready = false;
    if (!delivered) la_mdot_seg(ctx, r, 0, 1, zz, sg, slot_rz);
  };
  pc_and_rz(p, sRZc, first_x0_ready && pre.on);
  PPH_TRY(la_reduce_device(ctx, sRZc, 1));
  for (int it = 0; it < its; ++it) {
    const bool last = (it == its - 1);
    if (it > 0) {
      pc_and_rz(z, sRZn, pre.on);
      PPH_TRY(la_reduce_device(ctx, sRZn, 1));
      la_p_update_dev(ctx, p, z, sRZn, sRZc, n);
    }
    la_spmv_dot(ctx, A, p, q, sPQ, it > 0 ? sRZn : -1, sRZc);
    PPH_TRY(la_reduce_device(ctx, sPQ, 1));
    la_cg_update_dev(ctx, x, r, p, q, sRZc, sPQ, n, sRR, sg, (pre.on && !last) ? z : nullptr, pre.dinv, pre.w, S_BAD);
    PPH_TRY(la_reduce_device(ctx, sRR, 1));
  }
  // (a breakdown - p.Ap zero or NaN - is counted in scal[S_BAD] by the update kernel; the Picard loop publishes the count
  // with the sweep's norms and reports it as inner_failed)
  out->its = its; out->res = -1.0; out->converged = true; out->breakdown = false; out->bnorm = -1.0;
  return PPH_OK;
}

static int cg_solve(pph_ctx* ctx, const Csr& A, const double* b, double* x, const double* dinv, const ApplyFn& pc,
                    double rtol, double atol, int max_it, bool warm, double* r, double* z, double* p, double* q,
                    int slot, KspOut* out, double* hist, int hist_cap, double bnorm_hint = -1.0,
                    double reduction = 0.0, const double* r_init = nullptr, int norm_type = 0,
                    const MgPre& pre = MgPre(), double rnorm_hint = -1.0, bool first_x0_ready = false,
                    CgMemo* memo = nullptr, bool x_is_zero = false) {   // x_is_zero: a cold solve's x already holds zeros
  const int64_t n = A.nrows;
  if (norm_type == 2 && la_device_scalars(ctx))
    return cg_solve_fixed(ctx, A, b, x, dinv, pc, max_it, warm, r, z, p, q, slot, out, r_init, pre, first_x0_ready && warm && r_init,
                          x_is_zero);
  if (norm_type == 2) {
    // host-scalar transport: the natural-norm loop with an unreachable tolerance does the same iterations
    const int st = cg_solve_natural(ctx, A, b, x, dinv, pc, 0.0, 0.0, max_it, warm, r, z, p, q, slot, out, hist, hist_cap,
                                    1.0, 0.0, r_init, pre, -1.0, false, nullptr, x_is_zero);
    out->converged = !out->breakdown;
    return st;
  }
  if (norm_type == 1)
    return cg_solve_natural(ctx, A, b, x, dinv, pc, rtol, atol, max_it, warm, r, z, p, q, slot, out, hist, hist_cap,
                            bnorm_hint, reduction, r_init, pre, rnorm_hint, first_x0_ready && warm && r_init, memo, x_is_zero);
  // reductions run over the owned entries of a slab (whole vector on a single GPU)
  const Seg sg = pph_owned_seg(A.geom, n);
  const bool fused = (dinv != nullptr) || !pc;
  auto apply_pc = [&](const double* in, double* o) {
    if (dinv) la_pointwise_mult(ctx, o, dinv, in, n);
    else if (pc) pc(in, o);
    else la_copy(ctx, o, in, n);
  };
  double bnorm;
  if (warm) {
    // tolerance is relative to ||P^-1 b|| also with a non-zero guess (KSPConvergedDefault); callers that
    // solve a sequence of nearby systems pass the norm of the first one instead of paying a
    // preconditioner application per solve
    if (bnorm_hint > 0.0) {
      bnorm = bnorm_hint;
    } else {
      apply_pc(b, z);
      la_mdot_seg(ctx, z, 0, 1, z, sg, slot);
      PPH_TRY(la_fetch(ctx, slot, 1));
      bnorm = std::sqrt(ctx->h_scal[slot]);
    }
    // r_init: the caller already knows b - A x (residual bookkeeping of the Picard sweeps)
    if (r_init) { if (r_init != r) la_copy(ctx, r, r_init, n); }
    else la_spmv_resid(ctx, A, x, b, r);
  } else {
    if (!x_is_zero) la_set(ctx, x, 0.0, n);
    la_copy(ctx, r, b, n);
    bnorm = -1.0;
  }
  apply_pc(r, z);
  la_dot2_seg(ctx, r, z, z, sg, slot);
  PPH_TRY(la_fetch(ctx, slot, 2));
  double rz = ctx->h_scal[slot];
  double res = std::sqrt(ctx->h_scal[slot + 1]);
  if (bnorm < 0.0) bnorm = res;
  // `reduction` > 0: also accept a drop by that factor from the initial residual of THIS solve
  const double tol = std::fmax(std::fmax(rtol * bnorm, atol), reduction > 0.0 ? reduction * res : 0.0);
  out->its = 0; out->res = res; out->converged = false; out->breakdown = false; out->bnorm = bnorm;
  if (hist && hist_cap > 0) hist[0] = res;
  if (!(res == res)) { out->breakdown = true; return PPH_OK; }
  if (res <= tol) { out->converged = true; return PPH_OK; }
  la_copy(ctx, p, z, n);
  int its = 0;
  while (its < max_it) {
    la_spmv_dot(ctx, A, p, q, slot);
    PPH_TRY(la_fetch(ctx, slot, 1));
    const double pq = ctx->h_scal[slot];
    if (!(pq > 0.0) || !(rz == rz)) { out->breakdown = true; break; }
    const double alpha = rz / pq;
    double rz_new;
    if (fused) {
      la_cg_update(ctx, x, r, z, p, q, dinv, alpha, n, slot, sg);
    } else {
      la_axpy(ctx, x, alpha, p, n);
      la_axpy(ctx, r, -alpha, q, n);
      pc(r, z);
      la_dot2_seg(ctx, r, z, z, sg, slot);
    }
    PPH_TRY(la_fetch(ctx, slot, 2));
    rz_new = ctx->h_scal[slot];
    res = std::sqrt(ctx->h_scal[slot + 1]);
    ++its;
    if (hist && its < hist_cap) hist[its] = res;
    if (!(res == res)) { out->breakdown = true; break; }
    if (res <= tol) { out->converged = true; break; }
    const double beta = rz_new / rz;
    la_axpby(ctx, p, 1.0, z, beta, n);
    rz = rz_new;
  }
  out->its = its;
  out->res = res;
  return PPH_OK;
}

int pph_cg_jacobi(pph_ctx* ctx, const Csr& A, const double* b, double* x, const double* dinv, double rtol, double atol,
                  int max_it, double* r, double* z, double* p, double* q, int* its) {
  KspOut ko;
  PPH_TRY(cg_solve(ctx, A, b, x, dinv, ApplyFn(), rtol, atol, max_it, false, r, z, p, q, S_COARSE, &ko, nullptr, 0));
  if (its) *its = ko.its;
  if (!ko.converged || ko.breakdown) ctx->coarse_failed++;   // reported as pph_solve_info.inner_failed
  return PPH_OK;
}

// ------------------------------------------------------------------------------------------------
// left-preconditioned restarted GMRES, classical Gram-Schmidt (one fused multi-dot + one multi-axpy
// per step), Givens recurrence on the host
// ------------------------------------------------------------------------------------------------
// work vectors and reduction slots of one GMRES instance (the block solves run one inside the outer one's PC)
struct GmresWs { int idV, idW, idT, sA, sMD; };
static const GmresWs GMRES_OUTER = {W_GV, W_GW, W_GT, S_A, S_MDOT};
static const GmresWs GMRES_INNER = {W_IGV, W_IGW, W_IGT, S_INNER, S_MDOT + 64};

static int gmres_solve(pph_ctx* ctx, const ApplyFn& Aop, int64_t n, const double* b, double* x, const ApplyFn& pc,
                       int restart, double rtol, double atol, int max_it, KspOut* out, double* hist, int hist_cap,
                       Seg sg, const GmresWs& ws = GMRES_OUTER) {
  const int S_A = ws.sA, S_MDOT = ws.sMD;   // (shadow the outer instance's slots)
  double *V, *w, *t;
  PPH_TRY(work(ctx, ws.idV, (size_t)(restart + 1) * (size_t)n, &V));
  PPH_TRY(work(ctx, ws.idW, (size_t)n, &w));
  PPH_TRY(work(ctx, ws.idT, (size_t)n, &t));
  auto apply_pc = [&](const double* in, double* o) {
    if (pc) pc(in, o); else la_copy(ctx, o, in, n);
  };
  std::vector<double> H((size_t)(restart + 1) * restart, 0.0), cs(restart), sn(restart), g(restart + 1), y(restart),
      hcol(restart + 2);
  auto Hat = [&](int i, int k) -> double& { return H[(size_t)k * (restart + 1) + i]; };
  la_set(ctx, x, 0.0, n);
  // r0 = P^-1 b  (zero initial guess)
  apply_pc(b, V);
  la_mdot_seg(ctx, V, 0, 1, V, sg, S_A);
  PPH_TRY(la_fetch(ctx, S_A, 1));
  double beta = std::sqrt(ctx->h_scal[S_A]);
  const double tol = std::fmax(rtol * beta, atol);
  out->its = 0; out->res = beta; out->converged = false; out->breakdown = false;
  if (hist && hist_cap > 0) hist[0] = beta;
  if (!(beta == beta)) { out->breakdown = true; return PPH_OK; }
  if (beta <= tol) { out->converged = true; return PPH_OK; }
  int its = 0;
  double res = beta;
  bool first = true;
  while (its < max_it) {
    if (!first) {
      // r = P^-1 (b - A x)
      Aop(x, t);
      la_sub(ctx, t, b, t, n);
      apply_pc(t, V);
      la_mdot_seg(ctx, V, 0, 1, V, sg, S_A);
      PPH_TRY(la_fetch(ctx, S_A, 1));
      beta = std::sqrt(ctx->h_scal[S_A]);
    }
    first = false;
    la_scale(ctx, V, 1.0 / beta, n);
    std::fill(g.begin(), g.end(), 0.0);
    g[0] = beta;
    int kused = 0;
    bool done = false;
    for (int k = 0; k < restart; ++k) {
      double* vk = V + (size_t)k * n;
      double* vk1 = V + (size_t)(k + 1) * n;
      Aop(vk, t);
      apply_pc(t, w);
      la_mdot_seg(ctx, V, n, k + 1, w, sg, S_MDOT);
      PPH_TRY(la_fetch(ctx, S_MDOT, k + 1));
      for (int i = 0; i <= k; ++i) hcol[i] = ctx->h_scal[S_MDOT + i];
      la_maxpy_neg(ctx, w, V, n, k + 1, hcol.data(), n);
      la_mdot_seg(ctx, w, 0, 1, w, sg, S_A);
      PPH_TRY(la_fetch(ctx, S_A, 1));
      const double hn = std::sqrt(ctx->h_scal[S_A]);
      for (int i = 0; i <= k; ++i) Hat(i, k) = hcol[i];
      Hat(k + 1, k) = hn;
      if (hn > 0.0) {
        la_copy(ctx, vk1, w, n);
        la_scale(ctx, vk1, 1.0 / hn, n);
      }
      for (int i = 0; i < k; ++i) {
        const double tmp = cs[i] * Hat(i, k) + sn[i] * Hat(i + 1, k);
        Hat(i + 1, k) = -sn[i] * Hat(i, k) + cs[i] * Hat(i + 1, k);
        Hat(i, k) = tmp;
      }
      const double d = std::hypot(Hat(k, k), Hat(k + 1, k));
      if (!(d > 0.0) || !(d == d)) { out->breakdown = true; done = true; kused = k; break; }
      cs[k] = Hat(k, k) / d;
      sn[k] = Hat(k + 1, k) / d;
      Hat(k, k) = d;
      Hat(k + 1, k) = 0.0;
      g[k + 1] = -sn[k] * g[k];
      g[k] = cs[k] * g[k];
      ++its;
      kused = k + 1;
      res = std::fabs(g[k + 1]);
      if (hist && its < hist_cap) hist[its] = res;
      if (res <= tol || its >= max_it) { done = true; break; }
    }
    // back substitution and update
    for (int i = kused - 1; i >= 0; --i) {
      double s = g[i];
      for (int j = i + 1; j < kused; ++j) s -= Hat(i, j) * y[j];
      y[i] = s / Hat(i, i);
    }
    if (kused > 0) la_maxpy(ctx, x, V, n, kused, y.data(), n);
    if (done) break;
  }
  out->its = its;
  out->res = res;
  out->converged = (res <= tol) && !out->breakdown;
  return PPH_OK;
}

// ------------------------------------------------------------------------------------------------
// preconditioner data
// ------------------------------------------------------------------------------------------------
__global__ void k_block2_build(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                               const double* __restrict__ A11, const double* __restrict__ A22,
                               const double* __restrict__ A12, const double* __restrict__ A21, int64_t n,
                               double* __restrict__ binv) {
  for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = rowptr[row], hi = rowptr[row + 1] - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)col[mid] < row) lo = mid + 1; else hi = mid;
    }
    const double d11 = A11[lo], d22 = A22[lo], d12 = A12[lo], d21 = A21[lo];
    const double det = d11 * d22 - d12 * d21;
    if (det == 0.0) {  // empty (ghost) rows: identity
      binv[row] = 1.0; binv[n + row] = 0.0; binv[2 * n + row] = 0.0; binv[3 * n + row] = 1.0;
      continue;
    }
    const double r = 1.0 / det;
    binv[row] = d22 * r;          // z1 <- r1
    binv[n + row] = -d12 * r;     // z1 <- r2
    binv[2 * n + row] = -d21 * r; // z2 <- r1
    binv[3 * n + row] = d11 * r;  // z2 <- r2
  }
}

struct BlockSolver {
  // solves A_which z = rhs for one scalar block with an inner preconditioned CG
  pph_ctx* ctx;
  const pph_solver_cfg* cfg;
  Csr A[2];
  double* dinv[2] = {nullptr, nullptr};
  int total_its = 0;
  bool failed = false;
  bool onchip_used = false;              // an on-chip block solve ran: its record is read when the solve ends
  double bnorm_cache[2] = {-1.0, -1.0};  // ||P^-1 b|| of the first (cold) solve of each block
  double* last_resid = nullptr;          // recurrence residual rhs - A z of the last CG solve (work vector)
  CgMemo memo[2];                        // per block, of this pph_solve_device call (option "presmooth_lazy")

  int setup() {
    A[0] = block_csr(ctx, 0);
    A[1] = block_csr(ctx, 1);
    if (cfg->inner_pc_type == PPH_PC_JACOBI) {
      if (ctx->diag0_valid) {   // the fused assembly produced 1 / a_ii of both diagonal blocks
        dinv[0] = ctx->dinv0[0].p;
        dinv[1] = ctx->dinv0[1].p;
      } else {
        PPH_TRY(pph_ensure_csr_blocks(ctx));
        A[0] = block_csr(ctx, 0);
        A[1] = block_csr(ctx, 1);
        PPH_TRY(work(ctx, W_DINV_1, (size_t)ctx->n, &dinv[0]));
        PPH_TRY(work(ctx, W_DINV_2, (size_t)ctx->n, &dinv[1]));
        la_extract_diag_inv(ctx, A[0], dinv[0]);
        la_extract_diag_inv(ctx, A[1], dinv[1]);
      }
    } else if (cfg->inner_pc_type == PPH_PC_MG || cfg->inner_pc_type == PPH_PC_PMG) {
      // (PPH_PC_PMG reaches this point on degree-2 contexts only: mg_setup puts their operator on top of the CG-1 hierarchy)
      PPH_TRY(mg_setup(ctx));
    } else if (cfg->inner_pc_type == PPH_PC_ILU) {
      // ILU(0) of both diagonal blocks (CSR values needed: the fused assembly keeps stencil-ELL copies only)
      PPH_TRY(pph_ensure_csr_blocks(ctx));
      A[0] = block_csr(ctx, 0);
      A[1] = block_csr(ctx, 1);
      for (int f = 0; f < 2; ++f)
        if (!ctx->ilu[1 + f].valid) PPH_TRY(ilu_factor(ctx, ctx->ilu[1 + f], A[f]));
    } else if (cfg->inner_pc_type != PPH_PC_NONE) {
      pph_set_error(ctx, "inner pc_type %d not supported for block solves (none, jacobi, mg, pph_pmg, ilu)", cfg->inner_pc_type);
      return PPH_ERR_INVALID;
    }
    return PPH_OK;
  }

  // r_io (optional): vector the CG uses as its residual - on entry b - A z when warm and r_known, on return the
  // recurrence residual of the solve (the Picard loop keeps its block residuals there: no copies in or out)
  // rnorm_hint >= 0: ||r_init|| over the owned rows, known to the caller.  last_res: residual norm the block's CG ended
  // with (unpreconditioned-norm CG only; -1 otherwise)
  double last_res = -1.0;
  // where a caller that produces the residual a warm CG solve of block `which` starts from may leave its first
  // pre-smoothing z0 = dinv .* r * w (then: solve(..., z0_ready = true)); false: this solve has no use for it
  bool presmooth_target(int which, double** z0, const double** d, const double** w, const SellDict** dd) {
    if (cfg->inner_ksp_type != PPH_KSP_CG || cfg->inner_pc_type != PPH_PC_MG || cfg->inner_norm == 0 || !A[which].ell.val) return false;
    const int ns = cfg->mg_smooth > 0 ? cfg->mg_smooth : 2;
    bool lo = false;
    if (!mg_pre_smoother(ctx, which, ns, d, w, &lo, dd)) return false;
    return work(ctx, W_IP, (size_t)ctx->n, z0) == PPH_OK;
  }
  int solve(int which, const double* rhs, double* z, bool warm, const double* r_init = nullptr, double* r_io = nullptr,
            double rnorm_hint = -1.0, bool z0_ready = false, bool z_is_zero = false) {   // z_is_zero: cold solve, z already zeroed
    last_res = -1.0;
    const int64_t n = ctx->n;
    double *r, *zz, *p, *q;
    PPH_TRY(work(ctx, W_IR, (size_t)n, &r));
    if (r_io) r = r_io;
    PPH_TRY(work(ctx, W_IZ, (size_t)n, &zz));
    PPH_TRY(work(ctx, W_IP, (size_t)n, &p));
    PPH_TRY(work(ctx, W_IQ, (size_t)n, &q));
    ApplyFn pc;
    const int ns = cfg->mg_smooth > 0 ? cfg->mg_smooth : 2;
    if (cfg->inner_pc_type == PPH_PC_MG || cfg->inner_pc_type == PPH_PC_PMG)
      pc = [this, which, ns](const double* in, double* o) { mg_vcycle(ctx, which, in, o, ns); };
    if (cfg->inner_pc_type == PPH_PC_ILU)
      pc = [this, which](const double* in, double* o) { if (ilu_apply(ctx, ctx->ilu[1 + which], in, o) < 0) failed = true; };
    KspOut ko;
    if (cfg->inner_exact && !cfg->picard && ctx->world == 1 && n <= 4096 && A[which].ell.val && ctx->diag0_valid && !warm) {
      // the reference's LU block on a plumbing-size mesh (16 x 16: 289 rows): the whole block solve inside one workgroup,
      // Jacobi-CG to inner_rtol on chip - one launch instead of ~9 host-driven multigrid-CG iterations of ~10 launches and
      // one round trip each (BASELINE config 1 through solve_dpp: 20 -> ~2 ms)
      // How each of these solves ended is not looked at here (that would be the round trip this path exists to avoid): the
      // kernel adds to ctx->onchip_rec, which pph_solve_device reads once, after its final synchronisation.  A solve that
      // stops short is REPORTED (inner_failed), not repeated on the host-driven loop.
      if (!onchip_used) {
        PPH_HIP(ctx, hipMemsetAsync(ctx->onchip_rec.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
        onchip_used = true;
      }
      mg_onchip_cg(ctx, A[which].ell, ctx->dinv0[which].p, rhs, z, r, p, q, n, cfg->inner_rtol < 1e-12 ? cfg->inner_rtol : 1e-12,
                   ctx->onchip_max_it > 0 ? ctx->onchip_max_it : 8 * (int)n + 64, ctx->onchip_rec.p);
      last_resid = nullptr;
      total_its += 1;
      return PPH_OK;
    }
    if (cfg->inner_ksp_type == PPH_KSP_PREONLY) {
      // one application of the inner preconditioner
      if (dinv[which]) la_pointwise_mult(ctx, z, dinv[which], rhs, n);
      else if (pc) pc(rhs, z);
      else la_copy(ctx, z, rhs, n);
      return PPH_OK;
    }
    if (cfg->inner_ksp_type == PPH_KSP_GMRES) {
      // restarted GMRES on the block (FIELDSPLIT_GMRES*_PARAMS); a warm start solves for the correction
      const Csr& Ab = A[which];
      ApplyFn Aop = [this, &Ab](const double* xx, double* yy) { la_spmv(ctx, Ab, xx, yy); };
      ApplyFn pcj = pc;
      if (dinv[which]) { const double* dj = dinv[which]; pcj = [this, dj, n](const double* in, double* o) { la_pointwise_mult(ctx, o, dj, in, n); }; }
      const Seg sg = pph_owned_seg(Ab.geom, n);
      if (!warm) {
        PPH_TRY(gmres_solve(ctx, Aop, n, rhs, z, pcj, 30, cfg->inner_rtol, cfg->inner_atol, cfg->inner_max_it, &ko, nullptr, 0,
                            sg, GMRES_INNER));
      } else {
        double* rr;
        PPH_TRY(work(ctx, W_IGR, (size_t)n, &rr));
        la_spmv_resid(ctx, Ab, z, rhs, rr);
        PPH_TRY(gmres_solve(ctx, Aop, n, rr, zz, pcj, 30, cfg->inner_rtol, cfg->inner_atol, cfg->inner_max_it, &ko, nullptr, 0,
                            sg, GMRES_INNER));
        la_axpy(ctx, z, 1.0, zz, n);
      }
      last_resid = nullptr;
      total_its += ko.its;
      if (ko.breakdown || !ko.converged) failed = true;
      return PPH_OK;
    }
    MgPre pre;
    if (cfg->inner_pc_type == PPH_PC_MG) pre.on = mg_pre_smoother(ctx, which, ns, &pre.dinv, &pre.w, &pre.launch_only);
    pre.tag = 16 * ns + which;
    PPH_TRY(cg_solve(ctx, A[which], rhs, z, dinv[which], pc, cfg->inner_rtol, cfg->inner_atol, cfg->inner_max_it,
                     warm, r, zz, p, q, S_INNER, &ko, nullptr, 0, warm ? bnorm_cache[which] : -1.0,
                     cfg->inner_reduction, warm ? r_init : nullptr, cfg->inner_norm, pre, rnorm_hint, z0_ready, &memo[which],
                     z_is_zero && !warm));
    if (!warm) bnorm_cache[which] = ko.bnorm;
    if (cfg->inner_norm == 1) last_res = ko.res;
    last_resid = r;
    total_its += ko.its;
    if (ko.breakdown || !ko.converged) failed = true;
    return PPH_OK;
  }
};

// ------------------------------------------------------------------------------------------------
// the solve entry point
// ------------------------------------------------------------------------------------------------
__global__ void k_add2(double* __restrict__ out, const double* __restrict__ a, const double* __restrict__ b,
                       int64_t n, int desc) {   // (desc: option l3_order, PPH_DIR_LOOP in pph_internal.h)
  PPH_DIR_LOOP(i, n, desc) out[i] = a[i] + b[i];
}

int validate_cfg(pph_ctx* ctx, const pph_solver_cfg* cfg) {   // (also pph_solve_rhs*, pph_adjoint.hip)
  PPH_REQUIRE(ctx, cfg != nullptr, "solver cfg is NULL");
  PPH_REQUIRE(ctx, cfg->ksp_type >= PPH_KSP_PREONLY && cfg->ksp_type <= PPH_KSP_GMRES, "unknown ksp_type %d",
              cfg->ksp_type);
  PPH_REQUIRE(ctx, cfg->pc_type >= PPH_PC_NONE && cfg->pc_type <= PPH_PC_CMG, "unknown pc_type %d", cfg->pc_type);
  // the coupled cycle preconditions the monolithic system, on one context with a CG-1 hierarchy
  PPH_REQUIRE(ctx, cfg->inner_pc_type != PPH_PC_CMG || !(cfg->pc_type == PPH_PC_FIELDSPLIT || cfg->picard),
              "pc_type pph_cmg is a cycle on the coupled system, not a block preconditioner: use it as pc_type of a monolithic solve");
  if (cfg->pc_type == PPH_PC_CMG) {
    PPH_REQUIRE(ctx, !cfg->picard, "pc_type pph_cmg preconditions the monolithic Krylov solve: not available with picard");
    PPH_REQUIRE(ctx, ctx->mesh.degree == 1,
                "pc_type pph_cmg runs on the CG-1 hierarchy: degree-2 spaces have none (a coupled pph_pmg does not exist)");
    PPH_REQUIRE(ctx, ctx->world == 1, "pc_type pph_cmg: single context only (no slab decomposition)");
  }
  PPH_REQUIRE(ctx, cfg->pc_type != PPH_PC_PMG, "pc_type pph_pmg applies to the scalar blocks: use it as inner_pc_type");
  // degree 2 has no multigrid hierarchy: pc mg, and block solves on it (which the LU blocks also stand for), are refused
  PPH_REQUIRE(ctx, ctx->mesh.degree == 1 || (cfg->pc_type != PPH_PC_MG &&
                   !((cfg->pc_type == PPH_PC_FIELDSPLIT || cfg->picard) && cfg->inner_pc_type == PPH_PC_MG)),
              "degree-2 spaces have no multigrid hierarchy: pc_type mg (also as the block pc of a field split / Picard sweep, "
              "and the LU blocks it stands for) is not available; use none, jacobi, pph_block2 or ilu");
  PPH_REQUIRE(ctx, !(cfg->pc_type == PPH_PC_ILU || cfg->inner_pc_type == PPH_PC_ILU) || ctx->world == 1,
              "pc_type ilu eliminates sequentially along the global row order: single context only");
  PPH_REQUIRE(ctx, cfg->restart >= 1 && cfg->restart <= 30, "GMRES restart %d outside [1,30]", cfg->restart);
  PPH_REQUIRE(ctx, cfg->max_it >= 0 && cfg->inner_max_it >= 0 && cfg->picard_max_it >= 0, "negative max_it");
  PPH_REQUIRE(ctx, cfg->rtol >= 0 && cfg->atol >= 0 && cfg->inner_rtol >= 0 && cfg->inner_atol >= 0, "negative tolerance");
  PPH_REQUIRE(ctx, cfg->inner_reduction >= 0 && cfg->inner_reduction < 1, "inner_reduction must be in [0,1)");
  PPH_REQUIRE(ctx, cfg->inner_norm >= 0 && cfg->inner_norm <= 2,
              "inner_norm must be 0 (preconditioned), 1 (unpreconditioned) or 2 (none: exactly inner_max_it iterations)");
  PPH_REQUIRE(ctx, cfg->inner_norm != 2 || (cfg->inner_ksp_type == PPH_KSP_CG && cfg->inner_max_it >= 1 && cfg->inner_max_it <= 1000),
              "inner_norm 2 (no convergence test) needs inner ksp_type cg and 1 <= inner_max_it <= 1000");
  PPH_REQUIRE(ctx, cfg->inner_ksp_type == PPH_KSP_PREONLY || cfg->inner_ksp_type == PPH_KSP_CG ||
                       cfg->inner_ksp_type == PPH_KSP_GMRES,
              "inner ksp_type %d not supported (preonly, cg, gmres)", cfg->inner_ksp_type);
  if (!cfg->picard) {
    PPH_REQUIRE(ctx, cfg->pc_type != PPH_PC_MG, "pc_type mg applies to the scalar blocks: use it as inner_pc_type");
    PPH_REQUIRE(ctx, ctx->mono_ok, "monolithic Krylov solve needs pph_assemble_dpp(..., monolithic=1)");
  }
  return PPH_OK;
}

int pph_solve_device(pph_ctx* ctx, const pph_solver_cfg* cfg, pph_solve_info* info, double* hist, int hist_cap) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, ctx->asm_ok, "pph_solve before pph_assemble_dpp");
  PPH_TRY(validate_cfg(ctx, cfg));
  // a degree-1 context has no p-level to add: there PPH_PC_PMG is PPH_PC_MG, path for path
  pph_solver_cfg cfg_mg;
  if (cfg->inner_pc_type == PPH_PC_PMG && ctx->mesh.degree == 1) {
    cfg_mg = *cfg;
    cfg_mg.inner_pc_type = PPH_PC_MG;
    cfg = &cfg_mg;
  }
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t n = ctx->n, N = 2 * n;
  la_reset_spmv_stats(ctx);
  ctx->n_halo = 0;
  ctx->n_allreduce = 0;
  ctx->n_split = 0;
  if (ctx->comm_status != PPH_OK) { ctx->err = ctx->comm_error; return ctx->comm_status; }
  PPH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));

  pph_solve_info inf;
  inf.iterations = 0; inf.inner_iterations = 0; inf.converged = 0; inf.inner_failed = 0; inf.resnorm = 0; inf.rhs_norm = 0;
  ctx->coarse_failed = 0;
  ctx->onchip_solves = ctx->onchip_unconverged = ctx->onchip_its = 0;
  ctx->n_presmooth_skipped = ctx->n_presmooth_late = ctx->n_presmooth_unused = 0;
  la_dot(ctx, ctx->rhs.p, ctx->rhs.p, N, S_A);
  PPH_TRY(la_fetch(ctx, S_A, 1));
  inf.rhs_norm = std::sqrt(ctx->h_scal[S_A]);

  double* du;
  PPH_TRY(work(ctx, W_DU, (size_t)N, &du));
  BlockSolver bs;
  bs.ctx = ctx; bs.cfg = cfg;
  const Csr A12 = block_csr(ctx, 2), A21 = block_csr(ctx, 3);
  int status = PPH_OK;

  if (cfg->picard) {
    // block Picard / fixed-stress sweeps on the correction du (homogeneous BCs):
    //   A11 du1 = b1 - A12 du2_old ;  A22 du2 = b2 - A21 du1_new        (dpp.py:196-203)
    PPH_TRY(bs.setup());
    double* pb;
    PPH_TRY(work(ctx, W_PB, (size_t)n, &pb));
    const double* b1 = ctx->rhs.p;
    const double* b2 = ctx->rhs.p + n;
    double* du1 = du;
    double* du2 = du + n;
    la_set(ctx, du, 0.0, N);
    const double r0 = inf.rhs_norm;
    const double tol = std::fmax(cfg->picard_rtol * r0, cfg->picard_atol);
    double res = r0;
    if (hist && hist_cap > 0) hist[0] = res;
    int its = 0;
    // Residual bookkeeping: R0 = b1 - A11 du1 - A12 du2 and R1 = b2 - A21 du1 - A22 du2 are carried along.
    // A block solve leaves its CG recurrence residual; when the other block moves, the residual changes by
    // the change of the coupling term, which the sweep computes anyway (t12 = A12 du2, rhs1 = b2 - A21 du1).
    // So a sweep costs two coupling SpMVs, the warm-started solves start from a known residual, and
    // ||(R0, R1)|| is the monolithic residual (confirmed once with a true residual at convergence).
    double *t12, *tn, *rhs1, *R0, *R1;
    PPH_TRY(work(ctx, W_T12, (size_t)n, &t12));
    PPH_TRY(work(ctx, W_TN, (size_t)n, &tn));
    PPH_TRY(work(ctx, W_RHS1, (size_t)n, &rhs1));
    PPH_TRY(work(ctx, W_R1, (size_t)n, &R0));
    PPH_TRY(work(ctx, W_R2, (size_t)n, &R1));
    la_set(ctx, t12, 0.0, n);
    la_set(ctx, ctx->scal.p + S_BAD, 0.0, 1);
    const bool recur = (cfg->inner_ksp_type == PPH_KSP_CG);
    const int64_t pob = ctx->mesh.own_begin(), pon = ctx->mesh.own_end() - ctx->mesh.own_begin();
    // true residual from direct products only: t12 = A12 du2 and rhs1 = b2 - A21 du1 were formed by SpMVs with
    // the current iterates in this sweep, so two more products (A11 du1, A22 du2) complete it
    const double* rhs0 = pb;   // right-hand side handed to the macro block's solves
    auto true_residual = [&]() -> int {
      la_sub(ctx, pb, b1, t12, n);
      rhs0 = pb;
      la_spmv_resid(ctx, bs.A[0], du1, pb, R0);
      la_spmv_resid(ctx, bs.A[1], du2, rhs1, R1);
      la_dot(ctx, R0 + pob, R0 + pob, pon, S_A);
      la_dot(ctx, R1 + pob, R1 + pob, pon, S_A + 1);
      PPH_TRY(la_fetch(ctx, S_A, 2));
      res = std::sqrt(ctx->h_scal[S_A] + ctx->h_scal[S_A + 1]);
      return PPH_OK;
    };
    // Block solves without a convergence test (inner_norm 2) make a warm sweep a pure launch sequence - block solve,
    // coupling product, residual bookkeeping, block solve, coupling product, the two norms, their publication:
    // identical from sweep to sweep, so it is captured once and replayed (single context), and the only host
    // decision per sweep is the outer convergence test.
    const bool launch_only = recur && cfg->inner_norm == 2 && cfg->inner_pc_type != PPH_PC_ILU && la_device_scalars(ctx) &&
                             ctx->world == 1 && ctx->fetch_spin && !ctx->time_spmv;
    double rn0 = -1.0;   // ||R0|| at the start of a warm sweep
    // the coupling products also write the first pre-smoothing of the block solve that follows them (fused cycle)
    double* z0p[2] = {nullptr, nullptr};
    const double *z0d[2] = {nullptr, nullptr}, *z0w[2] = {nullptr, nullptr};
    const SellDict* z0c[2] = {nullptr, nullptr};   // the dictionaries of A11 / A22 while usable: z0d are their 1 / a_ii
    bool z0r[2] = {false, false};   // block 0: written by the previous sweep's last product
    if (recur && A12.ell.val && A21.ell.val)
      for (int f = 0; f < 2; ++f)
        if (!bs.presmooth_target(f, &z0p[f], &z0d[f], &z0w[f], &z0c[f])) z0p[f] = nullptr;
    while (res > tol && its < cfg->picard_max_it) {
      const bool warm = its > 0;
      if (warm && launch_only) {
        auto sweep = [&]() -> int {
          // (the block solves start from the residuals R0 / R1: their right-hand sides are not read)
          PPH_TRY(bs.solve(0, pb, du1, true, R0, R0, -1.0, z0r[0]));
          la_spmv_shift(ctx, A21, du1, b2, R1, rhs1, tn, S_B, pob, pob + pon, z0p[1], z0d[1], z0w[1], z0c[1]);   // rhs1 = b2 - A21 du1 ; R1 follows
          PPH_TRY(bs.solve(1, rhs1, du2, true, R1, R1, -1.0, z0p[1] != nullptr));
          la_spmv_shift(ctx, A12, du2, nullptr, R0, t12, tn, S_A, pob, pob + pon, z0p[0], z0d[0], z0w[0], z0c[0]);    // t12 = A12 du2 ; R0 follows ; ||R0||^2
          z0r[0] = z0p[0] != nullptr;
          la_dot(ctx, R1 + pob, R1 + pob, pon, S_A + 1);
          la_publish(ctx, S_A, 4);   // ||R0||^2, ||R1||^2, (S_B), breakdowns counted by the block solves (S_BAD)
          return PPH_OK;
        };
        const int its_before = bs.total_its;
        if (ctx->use_graphs == 2) {   // (measured after the kernel work of round 2: the eager sweep is faster, 64^3 2.65 vs 2.80 ms - the host runs ahead of a launch-only sequence anyway; a replay only adds its start-up latency)
          GraphKey gk;
          gk.p[0] = du; gk.p[1] = R0; gk.p[2] = R1; gk.p[3] = t12; gk.p[4] = tn; gk.p[5] = rhs1; gk.p[6] = pb;
          gk.p[7] = bs.A[0].ell.val ? (const void*)bs.A[0].ell.val : (const void*)bs.A[0].val;
          gk.n = n; gk.slot = cfg->inner_max_it; gk.epoch = ctx->mg_epoch;
          gk.tag = 5000 + 64 * cfg->inner_pc_type + (cfg->mg_smooth > 0 ? cfg->mg_smooth : 2);
          PPH_TRY(la_run_graph(ctx, gk, sweep));
        } else {
          PPH_TRY(sweep());
        }
        if (bs.total_its == its_before) bs.total_its += 2 * cfg->inner_max_it;   // a replayed sweep: counted here
        PPH_TRY(la_wait_published(ctx));
        ++its;
        if (ctx->h_scal[S_BAD] != 0.0) bs.failed = true;
        res = std::sqrt(ctx->h_scal[S_A] + ctx->h_scal[S_A + 1]);
        if (hist && its < hist_cap) hist[its] = res;
        if (!(res == res)) break;
        if (res <= tol) {
          PPH_TRY(true_residual());
          if (hist && its < hist_cap) hist[its] = res;
        }
        continue;
      }
      // a warm CG block solve starts from its carried residual (R0 / R1) and a cached ||b||: its right-hand side is
      // not read; with the unpreconditioned-norm test the host also knows the residual norms already (hints)
      const bool hints = warm && recur && cfg->inner_norm == 1;
      // rhs of the macro block.  Cold sweep of the CG blocks: t12 = +0, and b - (+0) == b bit for bit (-0 included), so
      // the solve reads b1 itself instead of a copy; as before, the warm sweeps are handed what the last la_sub left
      if (!warm && recur) rhs0 = b1;
      else if (!recur) la_sub(ctx, pb, b1, t12, n);
      // (cold: du was zeroed above and nothing has written the block since)
      PPH_TRY(bs.solve(0, rhs0, du1, warm, (warm && recur) ? R0 : nullptr, recur ? R0 : nullptr, hints ? rn0 : -1.0,
                       warm && z0r[0], !warm));
      double rn1 = -1.0;
      if (warm && recur) {
        // new rhs of the micro block, R1 += rhs1_new - rhs1_old, ||R1||^2 - one pass
        la_spmv_shift(ctx, A21, du1, b2, R1, rhs1, tn, S_B, pob, pob + pon, z0p[1], z0d[1], z0w[1], z0c[1]);
        if (hints) {
          PPH_TRY(la_fetch(ctx, S_B, 1));
          rn1 = std::sqrt(ctx->h_scal[S_B]);
        }
      } else {
        la_spmv_resid(ctx, A21, du1, b2, rhs1);
      }
      PPH_TRY(bs.solve(1, rhs1, du2, warm, (warm && recur) ? R1 : nullptr, recur ? R1 : nullptr, rn1,
                       warm && recur && z0p[1] != nullptr, !warm));
      ++its;
      if (recur) {
        // new coupling term, R0 += A12 du2_old - A12 du2_new, ||R0||^2 - one pass (the first sweep: t12 = 0)
        la_spmv_shift(ctx, A12, du2, nullptr, R0, t12, tn, S_A, pob, pob + pon, z0p[0], z0d[0], z0w[0], z0c[0]);
        z0r[0] = z0p[0] != nullptr;
        const double r1known = (cfg->inner_norm == 1) ? bs.last_res : -1.0;   // the CG's own final ||R1||
        if (r1known >= 0.0) {
          PPH_TRY(la_fetch(ctx, S_A, 1));
          ctx->h_scal[S_A + 1] = r1known * r1known;
        } else {
          la_dot(ctx, R1 + pob, R1 + pob, pon, S_A + 1);
          PPH_TRY(la_fetch(ctx, S_A, 2));
        }
        res = std::sqrt(ctx->h_scal[S_A] + ctx->h_scal[S_A + 1]);
        rn0 = std::sqrt(ctx->h_scal[S_A]);
      } else {
        la_spmv(ctx, A12, du2, tn);                                  // new coupling term
        la_copy(ctx, t12, tn, n);
        PPH_TRY(true_residual());
      }
      if (hist && its < hist_cap) hist[its] = res;
      if (!(res == res)) break;
      if (res <= tol && recur) {
        // confirm with the true residual once; keep sweeping if the recurrences were optimistic
        PPH_TRY(true_residual());
        if (hist && its < hist_cap) hist[its] = res;
      }
    }
    inf.iterations = its;
    inf.inner_iterations = bs.total_its;
    inf.resnorm = res;
    inf.converged = (res <= tol) ? 1 : 0;
    inf.inner_failed = (bs.failed || ctx->coarse_failed) ? 1 : 0;
    if (!inf.converged) status = PPH_ERR_DIVERGED;
  } else {
    const Csr A = mono_csr(ctx);
    ApplyFn Aop = [&](const double* x, double* y) { la_spmv(ctx, A, x, y); };
    ApplyFn pc;
    double* dinv = nullptr;
    if (cfg->pc_type == PPH_PC_JACOBI) {
      PPH_TRY(work(ctx, W_DINV_M, (size_t)N, &dinv));
      la_extract_diag_inv(ctx, A, dinv);
      pc = [&, dinv](const double* in, double* o) { la_pointwise_mult(ctx, o, dinv, in, N); };
    } else if (cfg->pc_type == PPH_PC_BLOCK2) {
      double* binv;
      PPH_TRY(pph_ensure_csr_blocks(ctx));
      PPH_TRY(work(ctx, W_BINV, (size_t)(4 * n), &binv));
      int grid = (int)(ceil_div64(n, 256) < 2048 ? ceil_div64(n, 256) : 2048);
      hipLaunchKernelGGL(k_block2_build, dim3(grid), dim3(256), 0, ctx->stream, ctx->mesh.rowptr.p, ctx->mesh.col.p,
                         ctx->A11.p, ctx->A22.p, ctx->A12.p, ctx->A21p(), n, binv);
      pc = [&, binv](const double* in, double* o) { la_block2_apply(ctx, o, binv, in, n); };
    } else if (cfg->pc_type == PPH_PC_CMG) {
      // one coupled multigrid cycle per application (pph_cmg.hip)
      PPH_TRY(cmg_setup(ctx));
      PPH_TRY(cmg_collect_failures(ctx));   // what an earlier application outside a solve left in the record is not this solve's
      ctx->coarse_failed = 0;
      const int ns = cfg->mg_smooth;
      pc = [&, ns](const double* in, double* o) { if (cmg_apply(ctx, in, o, ns) < 0) bs.failed = true; };
    } else if (cfg->pc_type == PPH_PC_ILU) {
      // ILU(0) of the monolithic field-major CSR (GMRES_ILU_PARAMS, parameters.py:27)
      if (!ctx->ilu[0].valid) PPH_TRY(ilu_factor(ctx, ctx->ilu[0], A));
      pc = [&](const double* in, double* o) { if (ilu_apply(ctx, ctx->ilu[0], in, o) < 0) bs.failed = true; };
    } else if (cfg->pc_type == PPH_PC_FIELDSPLIT) {
      // multiplicative: z1 = A11^-1 r1 ; z2 = A22^-1 (r2 - A21 z1)   (parameters.py:30-37)
      PPH_TRY(bs.setup());
      double *f1, *f2;
      PPH_TRY(work(ctx, W_FS1, (size_t)n, &f1));
      PPH_TRY(work(ctx, W_FS2, (size_t)n, &f2));
      pc = [&, f1, f2](const double* in, double* o) {
        bs.solve(0, in, o, false);
        la_spmv(ctx, A21, o, f1);
        la_sub(ctx, f2, in + n, f1, n);
        bs.solve(1, f2, o + n, false);
      };
    }
    KspOut ko;
    if (cfg->ksp_type == PPH_KSP_PREONLY) {
      if (pc) pc(ctx->rhs.p, du); else la_copy(ctx, du, ctx->rhs.p, N);
      ko.its = 1; ko.res = 0.0; ko.converged = true;
    } else if (cfg->ksp_type == PPH_KSP_CG) {
      double *r, *z, *p, *q;
      PPH_TRY(work(ctx, W_R, (size_t)N, &r));
      PPH_TRY(work(ctx, W_Z, (size_t)N, &z));
      PPH_TRY(work(ctx, W_P, (size_t)N, &p));
      PPH_TRY(work(ctx, W_Q, (size_t)N, &q));
      PPH_TRY(cg_solve(ctx, A, ctx->rhs.p, du, dinv, dinv ? ApplyFn() : pc, cfg->rtol, cfg->atol, cfg->max_it, false,
                       r, z, p, q, S_B, &ko, hist, hist_cap));
    } else {
      PPH_TRY(gmres_solve(ctx, Aop, N, ctx->rhs.p, du, pc, cfg->restart, cfg->rtol, cfg->atol, cfg->max_it, &ko, hist,
                          hist_cap, pph_owned_seg(A.geom, N)));
    }
    if (cfg->pc_type == PPH_PC_CMG) PPH_TRY(cmg_collect_failures(ctx));   // coarsest solves on the device that stopped short
    inf.iterations = ko.its;
    inf.inner_iterations = bs.total_its;
    inf.resnorm = ko.res;
    inf.converged = (ko.converged && !bs.failed) ? 1 : 0;
    inf.inner_failed = (bs.failed || ctx->coarse_failed) ? 1 : 0;
    if (!ko.converged || ko.breakdown) status = PPH_ERR_DIVERGED;
  }

  // u = u0 + du
  {
    int grid = (int)(ceil_div64(N, 256) < 2048 ? ceil_div64(N, 256) : 2048);
    hipLaunchKernelGGL(k_add2, dim3(grid), dim3(256), 0, ctx->stream, ctx->sol.p, ctx->u0.p, du, N, l3_pick(ctx, N));
  }
  // the record of the on-chip block solves travels with the solve's last launches (pinned destination: no wait of its own)
  if (bs.onchip_used)
    PPH_HIP(ctx, hipMemcpyAsync(ctx->h_onchip, ctx->onchip_rec.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  PPH_HIP(ctx, hipEventSynchronize(ctx->ev1));
  if (bs.onchip_used) {
    ctx->onchip_solves = (int64_t)ctx->h_onchip[0];
    ctx->onchip_unconverged = (int64_t)ctx->h_onchip[1];
    ctx->onchip_its = (int64_t)ctx->h_onchip[2];
    if (ctx->onchip_unconverged > 0) { inf.inner_failed = 1; inf.converged = 0; }   // as bs.failed: the preconditioner was not the one asked for
  }
  float ms = 0.f;
  PPH_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  ctx->t_solve = ms;
  la_harvest_spmv_times(ctx);
  PPH_TRY(sell_dict_poll(ctx));   // a dictionary refused by its per-assembly check on the device is retired on the host too
  if (ctx->mg_lam_pending) PPH_TRY(mg_lam_host(ctx));   // (the bounds arrived long ago: this only checks them - a bad one is an error, not a diverged solve)
  PPH_HIP(ctx, hipGetLastError());
  if (info) *info = inf;
  if (ctx->comm_status != PPH_OK) { ctx->err = ctx->comm_error; return ctx->comm_status; }
  if (status == PPH_ERR_DIVERGED)
    pph_set_error(ctx, "solver did not converge: %d iterations, residual %.3e", inf.iterations, inf.resnorm);
  return status;
}

int pph_get_solution(pph_ctx* ctx, double* x_host) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, ctx->asm_ok && ctx->sol.p, "no solution available");
  PPH_REQUIRE(ctx, x_host != nullptr, "x_host is NULL");
  PPH_HIP(ctx, hipMemcpyAsync(x_host, ctx->sol.p, sizeof(double) * 2 * (size_t)ctx->n, hipMemcpyDeviceToHost,
                              ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PPH_OK;
}

// the solution into a caller-owned device buffer, enqueued on the context stream (la_copy: a kernel, not the runtime's
// device-to-device copy); no synchronisation - the caller orders its own work after the context stream
int pph_copy_solution_device(pph_ctx* ctx, double* dst, int64_t count) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, ctx->asm_ok && ctx->sol.p, "no solution available");
  PPH_REQUIRE(ctx, dst != nullptr, "dst is NULL");
  PPH_REQUIRE(ctx, count == 2 * ctx->n, "count %lld, the solution has %lld entries", (long long)count, (long long)(2 * ctx->n));
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  la_copy(ctx, dst, ctx->sol.p, count);
  PPH_HIP(ctx, hipGetLastError());
  return PPH_OK;
}

int pph_solve(pph_ctx* ctx, const pph_solver_cfg* cfg, double* x_host, pph_solve_info* info, double* hist,
              int hist_cap) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, x_host != nullptr, "x_host is NULL");
  int st = pph_solve_device(ctx, cfg, info, hist, hist_cap);
  if (st < 0 && st != PPH_ERR_DIVERGED) return st;
  PPH_TRY(pph_get_solution(ctx, x_host));
  return st;
}

// ---- one block preconditioner, applied to a caller's vector (parity checks of the cycle itself) ----------------------
int pc_apply_prepare(pph_ctx* ctx, int which, int* pc_type) {
  PPH_REQUIRE(ctx, ctx->asm_ok, "pph_pc_apply before pph_assemble_dpp");
  PPH_REQUIRE(ctx, which == 0 || which == 1, "pph_pc_apply: which must be 0 (A11) or 1 (A22)");
  PPH_REQUIRE(ctx, ctx->world == 1, "pph_pc_apply: single context only");
  PPH_REQUIRE(ctx, *pc_type == PPH_PC_JACOBI || *pc_type == PPH_PC_MG || *pc_type == PPH_PC_PMG || *pc_type == PPH_PC_ILU,
              "pph_pc_apply: pc_type %d is no block preconditioner (jacobi, mg, pph_pmg, ilu)", *pc_type);
  if (*pc_type == PPH_PC_PMG && ctx->mesh.degree == 1) *pc_type = PPH_PC_MG;
  PPH_REQUIRE(ctx, *pc_type != PPH_PC_MG || ctx->mesh.degree == 1,
              "degree-2 spaces have no CG-1-only multigrid hierarchy: pc_type mg is not available; use pph_pmg");
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  if (*pc_type == PPH_PC_MG || *pc_type == PPH_PC_PMG) PPH_TRY(mg_setup(ctx));
  else PPH_TRY(pph_ensure_csr_blocks(ctx));
  return PPH_OK;
}

int pc_apply_device(pph_ctx* ctx, int which, int pc_type, int ns, const double* r, double* z, double* dinv_work) {
  if (pc_type == PPH_PC_JACOBI) {
    la_extract_diag_inv(ctx, block_csr(ctx, which), dinv_work);
    la_pointwise_mult(ctx, z, dinv_work, r, ctx->n);
  } else if (pc_type == PPH_PC_ILU) {
    const Csr A = block_csr(ctx, which);
    if (!ctx->ilu[1 + which].valid) PPH_TRY(ilu_factor(ctx, ctx->ilu[1 + which], A));
    PPH_REQUIRE(ctx, ilu_apply(ctx, ctx->ilu[1 + which], r, z) >= 0, "pph_pc_apply: ILU(0) application failed");
  } else {
    mg_vcycle(ctx, which, r, z, ns);
  }
  return PPH_OK;
}

// ---- a preconditioner set up once and applied per step (pph_eig_pclanczos) -------------------------------------------------
// The block cases go through pc_apply_prepare / pc_apply_device; what pc_apply_device redoes per application (the Jacobi
// diagonal) is taken once here.  The monolithic cases are those of pph_solve_device (Jacobi, 2 x 2 block-Jacobi, ILU(0) on
// ctx->ilu[0]), with data of their own so that a later solve finds its work vectors untouched.
int pc_operator_prepare(pph_ctx* ctx, int which, int pc_type, int mg_smooth, const Csr* M, PcOperator* P, const char* fn) {
  PPH_REQUIRE(ctx, ctx->world == 1, "%s works on a single context (the whole operator on one device)", fn);
  PPH_REQUIRE(ctx, which == 0 || (which >= 2 && which <= 4),
              "%s: which must be 0 (monolithic), 2 (M), 3 (A11) or 4 (A22), the symmetric positive definite operators; got %d", fn, which);
  PPH_REQUIRE(ctx, pc_type != PPH_PC_NONE, "%s: pc_type none is the operator itself: use pph_extreme_eigenvalues", fn);
  PPH_REQUIRE(ctx, pc_type != PPH_PC_FIELDSPLIT,
              "%s: the multiplicative field split is not a symmetric preconditioner: B A has no Lanczos recurrence", fn);
  PPH_REQUIRE(ctx, which == 2 || ctx->asm_ok, "%s before pph_assemble_dpp", fn);
  const int64_t n = ctx->n;
  P->which = which; P->ns = mg_smooth > 0 ? mg_smooth : 2;
  P->nrows = which == 0 ? 2 * n : n;
  P->setup_ms = 0.0;
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const auto t0 = std::chrono::steady_clock::now();
  bool built = false;
  if (which == 3 || which == 4) {
    const int f = which - 3;
    PPH_REQUIRE(ctx, pc_type == PPH_PC_JACOBI || pc_type == PPH_PC_ILU || pc_type == PPH_PC_MG || pc_type == PPH_PC_PMG,
                "%s: pc_type %d is no symmetric preconditioner of a scalar block (jacobi, ilu, mg, pph_pmg)", fn, pc_type);
    built = ((pc_type == PPH_PC_MG || pc_type == PPH_PC_PMG) && !ctx->mg_ok) || (pc_type == PPH_PC_ILU && !ctx->ilu[1 + f].valid);
    PPH_TRY(pc_apply_prepare(ctx, f, &pc_type));
    if (pc_type == PPH_PC_JACOBI) {
      PPH_TRY(P->data.alloc(ctx, (size_t)n));
      la_extract_diag_inv(ctx, block_csr(ctx, f), P->data.p);
    } else if (pc_type == PPH_PC_ILU) {
      if (!ctx->ilu[1 + f].valid) PPH_TRY(ilu_factor(ctx, ctx->ilu[1 + f], block_csr(ctx, f)));
    }
    P->mask[0] = ctx->bcmask[f].p;
  } else if (which == 0) {
    PPH_REQUIRE(ctx, ctx->mono_ok, "%s: monolithic CSR not assembled (pph_assemble_dpp(..., monolithic=1))", fn);
    PPH_REQUIRE(ctx, pc_type == PPH_PC_JACOBI || pc_type == PPH_PC_BLOCK2 || pc_type == PPH_PC_ILU || pc_type == PPH_PC_CMG,
                "%s: pc_type %d is no symmetric preconditioner of the monolithic system (jacobi, pph_block2, ilu, pph_cmg)", fn, pc_type);
    const Csr A = mono_csr(ctx);
    if (pc_type == PPH_PC_CMG) {
      built = !(ctx->mg_ok && ctx->cmg_ok && ctx->cmg_epoch == ctx->mg_values_epoch);
      PPH_TRY(cmg_setup(ctx));
    } else if (pc_type == PPH_PC_JACOBI) {
      PPH_TRY(P->data.alloc(ctx, (size_t)(2 * n)));
      la_extract_diag_inv(ctx, A, P->data.p);
    } else if (pc_type == PPH_PC_BLOCK2) {
      PPH_TRY(pph_ensure_csr_blocks(ctx));
      PPH_TRY(P->data.alloc(ctx, (size_t)(4 * n)));
      const int grid = (int)(ceil_div64(n, 256) < 2048 ? ceil_div64(n, 256) : 2048);
      hipLaunchKernelGGL(k_block2_build, dim3(grid), dim3(256), 0, ctx->stream, ctx->mesh.rowptr.p, ctx->mesh.col.p,
                         ctx->A11.p, ctx->A22.p, ctx->A12.p, ctx->A21p(), n, P->data.p);
    } else {
      built = !ctx->ilu[0].valid;
      if (built) PPH_TRY(ilu_factor(ctx, ctx->ilu[0], A));
    }
    P->mask[0] = ctx->bcmask[0].p;
    P->mask[1] = ctx->bcmask[1].p;
  } else {
    PPH_REQUIRE(ctx, pc_type == PPH_PC_JACOBI, "%s: the mass matrix takes pc_type jacobi only; got %d", fn, pc_type);
    PPH_REQUIRE(ctx, M && M->val && M->nrows == n, "%s: the mass matrix needs its CSR values", fn);
    PPH_TRY(P->data.alloc(ctx, (size_t)n));
    la_extract_diag_inv(ctx, *M, P->data.p);
  }
  P->pc_type = pc_type;
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  PPH_HIP(ctx, hipGetLastError());
  if (built) P->setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return PPH_OK;
}

int pc_operator_apply(pph_ctx* ctx, const PcOperator& P, const double* r, double* z) {
  const int64_t n = ctx->n;
  if (P.pc_type == PPH_PC_JACOBI) {
    la_pointwise_mult(ctx, z, P.data.p, r, P.nrows);
    return PPH_OK;   // (r is 0 on the constrained rows, so is z)
  }
  if (P.which == 0) {
    if (P.pc_type == PPH_PC_CMG) return cmg_apply(ctx, r, z, P.ns);   // (0 on the constrained rows by construction)
    if (P.pc_type == PPH_PC_BLOCK2) la_block2_apply(ctx, z, P.data.p, r, n);
    else PPH_REQUIRE(ctx, ilu_apply(ctx, ctx->ilu[0], r, z) >= 0, "pph_preconditioned_extremes: ILU(0) application failed");
    pmg_zero_masked(ctx, z, P.mask[0], n);
    pmg_zero_masked(ctx, z + n, P.mask[1], n);
  } else {
    PPH_TRY(pc_apply_device(ctx, P.which - 3, P.pc_type, P.ns, r, z, nullptr));
    pmg_zero_masked(ctx, z, P.mask[0], n);
  }
  return PPH_OK;
}

int pph_pc_apply(pph_ctx* ctx, int which, int pc_type, int mg_smooth, const double* r_host, double* z_host) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, r_host && z_host, "NULL vector");
  PPH_TRY(pc_apply_prepare(ctx, which, &pc_type));
  ctx->n_dict_dinv = 0;   // (counts this application's launches, as a solve's)
  ctx->n_l3_desc = 0; ctx->l3_last = 0;
  const int64_t n = ctx->n;
  DevBuf<double> r, z, w;
  PPH_TRY(r.alloc(ctx, (size_t)n));
  PPH_TRY(z.alloc(ctx, (size_t)n));
  PPH_TRY(w.alloc(ctx, (size_t)n));
  PPH_HIP(ctx, hipMemcpyAsync(r.p, r_host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  pmg_zero_masked(ctx, r.p, ctx->bcmask[which].p, n);   // as the residuals of the Krylov loops: 0 on constrained rows
  const int st = pc_apply_device(ctx, which, pc_type, mg_smooth > 0 ? mg_smooth : 2, r.p, z.p, w.p);
  if (st == PPH_OK) {
    PPH_HIP(ctx, hipMemcpyAsync(z_host, z.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  }
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  PPH_HIP(ctx, hipGetLastError());
  r.release(); z.release(); w.release();
  return st;
}

// ---- one monolithic preconditioner, applied to a caller's vector of 2n (parity checks of the coupled cycle itself) -------
int pph_pc_apply_coupled(pph_ctx* ctx, int pc_type, int mg_smooth, const double* r_host, double* z_host) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, r_host && z_host, "NULL vector");
  PPH_REQUIRE(ctx, ctx->asm_ok, "pph_pc_apply_coupled before pph_assemble_dpp");
  PPH_REQUIRE(ctx, pc_type == PPH_PC_CMG || pc_type == PPH_PC_BLOCK2 || pc_type == PPH_PC_JACOBI,
              "pph_pc_apply_coupled: pc_type %d is no preconditioner of the coupled system applied here (pph_cmg, pph_block2, jacobi)",
              pc_type);
  PcOperator P;
  PPH_TRY(pc_operator_prepare(ctx, 0, pc_type, mg_smooth, nullptr, &P, "pph_pc_apply_coupled"));
  const int64_t n = ctx->n, N = 2 * n;
  DevBuf<double> r, z;
  PPH_TRY(r.alloc(ctx, (size_t)N));
  PPH_TRY(z.alloc(ctx, (size_t)N));
  PPH_HIP(ctx, hipMemcpyAsync(r.p, r_host, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, ctx->stream));
  pmg_zero_masked(ctx, r.p, ctx->bcmask[0].p, n);   // as the residuals of the Krylov loops: 0 on constrained rows
  pmg_zero_masked(ctx, r.p + n, ctx->bcmask[1].p, n);
  const int st = pc_operator_apply(ctx, P, r.p, z.p);
  if (pc_type == PPH_PC_CMG) PPH_TRY(cmg_collect_failures(ctx));   // (this entry point has nobody to report them to: the record is cleared)
  if (st == PPH_OK) PPH_HIP(ctx, hipMemcpyAsync(z_host, z.p, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  PPH_HIP(ctx, hipGetLastError());
  r.release(); z.release();
  return st;
}

// diagnostic (tools/cmg_probe.py): `reps` coupled cycles on a vector of ones, then `reps` fine-level smoothing passes of the
// row-walk kernel alone (without the products of the diagonal blocks before it), each series timed with one event pair
int pph_cmg_bench(pph_ctx* ctx, int mg_smooth, int reps, double* out4) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, out4 && reps >= 1, "pph_cmg_bench: needs reps >= 1 and an output array");
  PPH_REQUIRE(ctx, ctx->asm_ok && ctx->mono_ok, "pph_cmg_bench: needs the monolithic assembly");
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const auto t0 = std::chrono::steady_clock::now();
  PPH_TRY(cmg_setup(ctx));
  const int64_t n = ctx->n, N = 2 * n;
  const int ns = mg_smooth > 0 ? mg_smooth : 2;
  DevBuf<double> r, z;
  PPH_TRY(r.alloc(ctx, (size_t)N));
  PPH_TRY(z.alloc(ctx, (size_t)N));
  la_set(ctx, r.p, 1.0, N);
  PPH_TRY(cmg_apply(ctx, r.p, z.p, ns));   // warm-up
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out4[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  float ms = 0.f;
  PPH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  for (int i = 0; i < reps; ++i) PPH_TRY(cmg_apply(ctx, r.p, z.p, ns));
  PPH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  PPH_HIP(ctx, hipEventSynchronize(ctx->ev1));
  PPH_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  out4[0] = (double)ms / reps;
  out4[2] = cmg_step_bytes(ctx);
  PPH_TRY(cmg_step_bench(ctx, reps, &out4[1]));
  PPH_TRY(cmg_collect_failures(ctx));
  r.release(); z.release();
  PPH_HIP(ctx, hipGetLastError());
  return PPH_OK;
}

// diagnostic (tools/pmg_probe.py): `reps` applications of the block preconditioner to a vector of ones.
// out[0] ms per application, out[1] ms of it spent in the passes over the degree-2 level (PPH_PC_PMG on a degree-2 context,
// else 0), out[2] bytes those passes move per application (tile kernels only, else 0), out[3] ms of the set-up the
// call had to do (hierarchy / factorisation; 0 when it was up to date)
int pph_pc_bench(pph_ctx* ctx, int which, int pc_type, int mg_smooth, int reps, double* out4) {
  if (!ctx) return PPH_ERR_INVALID;
  PPH_REQUIRE(ctx, out4 && reps >= 1, "pph_pc_bench: needs reps >= 1 and an output array");
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const auto t0 = std::chrono::steady_clock::now();
  PPH_TRY(pc_apply_prepare(ctx, which, &pc_type));
  const int64_t n = ctx->n;
  const int ns = mg_smooth > 0 ? mg_smooth : 2;
  DevBuf<double> r, z, w;
  PPH_TRY(r.alloc(ctx, (size_t)n));
  PPH_TRY(z.alloc(ctx, (size_t)n));
  PPH_TRY(w.alloc(ctx, (size_t)n));
  la_set(ctx, r.p, 1.0, n);
  pmg_zero_masked(ctx, r.p, ctx->bcmask[which].p, n);
  PPH_TRY(pc_apply_device(ctx, which, pc_type, ns, r.p, z.p, w.p));   // warm-up: factorisation, host copies of the bounds
  PPH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out4[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (hipEvent_t& e : ctx->pmg_ev)
    if (!e) PPH_HIP(ctx, hipEventCreate(&e));
  const bool p2 = pc_type == PPH_PC_PMG;
  double ms_all = 0.0, ms_top = 0.0;
  ctx->n_pmg_pass = 0; ctx->pmg_bytes = 0.0;
  int st = PPH_OK;
  for (int i = 0; i < reps && st == PPH_OK; ++i) {
    ctx->pmg_time = p2;
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    st = pc_apply_device(ctx, which, pc_type, ns, r.p, z.p, w.p);
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    ctx->pmg_time = false;
    PPH_HIP(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    PPH_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ms_all += ms;
    if (p2) {
      PPH_HIP(ctx, hipEventElapsedTime(&ms, ctx->pmg_ev[0], ctx->pmg_ev[1]));
      ms_top += ms;
      PPH_HIP(ctx, hipEventElapsedTime(&ms, ctx->pmg_ev[2], ctx->pmg_ev[3]));
      ms_top += ms;
    }
  }
  out4[0] = ms_all / reps;
  out4[1] = ms_top / reps;
  out4[2] = ctx->pmg_bytes / reps;
  r.release(); z.release(); w.release();
  return st;
}
