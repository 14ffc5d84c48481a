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
enum { S_A = 0, S_B = 2, S_BAD = 3, S_INNER = 8, S_COARSE = 16, S_MDOT = 64 };   // S_BAD: breakdowns counted on the device (launch-only sweeps)

// work vector ids
enum {
  W_R = 0, W_Z, W_P, W_Q,               // outer CG
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

// ---- arguments of the Krylov drivers: default-initialised, filled by designated members at the call site ----
struct CgSystem {   // the system of a CG solve and the vectors it works in
  const Csr* A = nullptr;
  const double* b = nullptr;
  double* x = nullptr;
  const double* dinv = nullptr;   // Jacobi: 1 / a_ii (goes before pc)
  const ApplyFn* pc = nullptr;    // any other preconditioner (neither: none)
  double *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr;   // work vectors
  int slot = 0;                   // first of the reduction slots in ctx->scal the solve uses
};
struct CgStart {   // what a CG solve starts from
  bool warm = false;                // x holds a guess (cold: x = 0)
  const double* r_init = nullptr;   // warm: b - A x, known to the caller (Picard bookkeeping); may be the work vector r itself
  double rnorm_hint = -1.0;         // >= 0: ||r_init||_2 over the owned rows, known to the caller (unpreconditioned norm)
  double bnorm_hint = -1.0;         // > 0: the norm of the right-hand side of an earlier, nearby system (warm solves)
  bool x_is_zero = false;           // a cold solve's x already holds zeros
  bool first_x0_ready = false;      // who produced r_init also left the fused cycle's first pre-smoothing where p_0 goes
  bool resumes() const { return warm && r_init; }   // from a residual the caller supplies: the hints above hold only then
};
struct KspStop {   // when a Krylov solve stops and what it records on the way
  double rtol = 0.0, atol = 0.0;
  double reduction = 0.0;   // > 0: also accept a drop by that factor from the initial residual of THIS solve (CG)
  int max_it = 0;
  int norm_type = 0;        // CG: 0 preconditioned residual, 1 unpreconditioned, 2 none (exactly max_it iterations)
  double* hist = nullptr;   // residual norm per iteration
  int hist_cap = 0;
};

// z = M^-1 r: the inverse diagonal where there is one, else the preconditioner, else the identity
static void apply_pc(pph_ctx* ctx, const double* dinv, const ApplyFn* pc, const double* in, double* o, int64_t n) {
  if (dinv) la_pointwise_mult(ctx, o, dinv, in, n);
  else if (pc && *pc) (*pc)(in, o);
  else la_copy(ctx, o, in, n);
}

// The start-up the CG drivers share: x and r of a cold solve (x = 0, r = b) or a warm one (r = r_init, else b - A x), and
// before that, for a warm solve, the norm of the right-hand side its tolerance is relative to - norm_type 0: ||P^-1 b||
// (through z), 1: ||b||, 2: none wanted.  *bnorm < 0 on return: the driver takes the norm of its first residual (cold) or none.
static int cg_start(pph_ctx* ctx, const CgSystem& s, const CgStart& st, Seg sg, int norm_type, double* bnorm) {
  const int64_t n = s.A->nrows;
  *bnorm = -1.0;
  if (!st.warm) {
    if (!st.x_is_zero) la_set(ctx, s.x, 0.0, n);
    la_copy(ctx, s.r, s.b, n);
    return PPH_OK;
  }
  // tolerance is relative to ||P^-1 b|| also with a non-zero guess (KSPConvergedDefault); callers that
  // solve a sequence of nearby systems pass the norm of the first one instead of paying a
  // preconditioner application per solve
  if (norm_type != 2) {
    if (st.bnorm_hint > 0.0) {
      *bnorm = st.bnorm_hint;
    } else {
      if (norm_type == 0) {
        apply_pc(ctx, s.dinv, s.pc, s.b, s.z, n);
        la_mdot_seg(ctx, s.z, 0, 1, s.z, sg, s.slot);
      } else {
        la_mdot_seg(ctx, s.b, 0, 1, s.b, sg, s.slot);
      }
      PPH_TRY(la_fetch(ctx, s.slot, 1));
      *bnorm = std::sqrt(ctx->h_scal[s.slot]);
    }
  }
  if (st.r_init) { if (st.r_init != s.r) la_copy(ctx, s.r, st.r_init, n); }
  else la_spmv_resid(ctx, *s.A, s.x, s.b, s.r);
  return PPH_OK;
}

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

// ------------------------------------------------------------------------------------------------
// One CG iteration on device scalars (la_device_scalars): alpha and beta live in ctx->scal, in two halves around the
// point where a host that tests convergence does so.  Serves the tested loop (cg_solve_natural) and the fixed-count
// loop (cg_solve_fixed).  `host_tests`: the host sees p.Ap (breakdown test) and r.r (convergence test) once per
// iteration, in one copy - the final reductions of p.Ap and of the cycle's r.z are left to the kernels that consume them,
// the update can publish, slabs can merge their all-reduces.  Without it nothing of the solve reaches the host: the
// update kernel counts a breakdown (p.Ap zero or NaN) in scal[S_BAD] instead.
// ------------------------------------------------------------------------------------------------
struct CgDevice {
  pph_ctx* ctx;
  const CgSystem& s;
  const MgPre& pre;
  const Seg sg;
  const int64_t n;
  const bool host_tests;
  const int sPQ, sRR, sRZn, sRZc;   // p.Ap, r.r, r.z (new), r.z (current)
  // Slabs: ONE all-reduce behind the product instead of one for p.Ap and one for r.r (`merge_allreduce`, stencil-ELL
  // operators).  The product also sums r.Ap and Ap.Ap (mode 7); { p.Ap, r.Ap, Ap.Ap, local r.r of the PREVIOUS update }
  // sit in four consecutive slots and are summed over the ranks together; the host forms the new
  // r.r = r.r_prev - 2 alpha r.Ap + alpha^2 Ap.Ap - one step of the recurrence from a true value, no accumulation of
  // rounding - so an iteration costs two scalar all-reduces (r.z; this one) instead of three.
  const int sE;   // sE .. sE + 2 = p.Ap, r.Ap, Ap.Ap ; sE + 3 = r.r of the previous update
  const bool merged;
  bool published = false;   // (the publication of p.Ap and r.r rode on the update's final reduction)
  bool z_ready = false;     // the last update wrote the next cycle's pre-smoothed first guess into z

  CgDevice(pph_ctx* c, const CgSystem& sys, const MgPre& mp, Seg seg, bool tests)
      : ctx(c), s(sys), pre(mp), sg(seg), n(sys.A->nrows), host_tests(tests), sPQ(sys.slot), sRR(sys.slot + 1),
        sRZn(sys.slot + 2), sRZc(sys.slot + 3), sE(sys.slot + 4),
        merged(tests && c->merge_allreduce && c->world > 1 && !c->comm_suspended && sys.A->ell.val != nullptr) {}

  // zz = M^-1 r and r.z -> scal[slot_rz].  The hand-off to a fused multigrid cycle (pre.on; mg_vcycle_fused, pph_mg.hip):
  // before the application ctx->mg_dot_slot names the slot and ctx->mg_dot_seg the owned rows of a dot product the cycle
  // may deliver from its last kernel, and ctx->mg_x0_ready says that zz already holds the cycle's first pre-smoothing
  // dinv .* r * w (written by the CG update or by the caller's coupling product).  A cycle that delivered the dot product
  // leaves mg_dot_slot at -2; any other preconditioner leaves it alone, and the dot product is taken here.  Both fields
  // are back at "nothing asked" (-1, false) when this returns.
  void pc_and_rz(double* zz, int slot_rz, bool x0_ready) {
    if (pre.on) { ctx->mg_dot_slot = slot_rz; ctx->mg_dot_seg = sg; ctx->mg_x0_ready = x0_ready; }
    apply_pc(ctx, s.dinv, s.pc, s.r, zz, n);
    const bool delivered = ctx->mg_dot_slot == -2;
    ctx->mg_dot_slot = -1;
    ctx->mg_x0_ready = false;
    if (!delivered) la_mdot_seg(ctx, s.r, 0, 1, zz, sg, slot_rz);
  }
  // first direction p = z_0: written in place (x0_ready: pre-smoothed by the caller)
  int first_direction(bool x0_ready) {
    pc_and_rz(s.p, sRZc, x0_ready);
    PPH_TRY(la_reduce_device(ctx, sRZc, 1));
    return PPH_OK;
  }
  int direction() {
    if (host_tests) ctx->defer_next_final = true;   // (r.z of the cycle's last kernel: summed inside the direction update)
    if (pre.on && !z_ready) ctx->n_presmooth_late++;   // (the update before was predicted to be the last: k_cheb_init, same bits)
    pc_and_rz(s.z, sRZn, z_ready);
    ctx->defer_next_final = false;
    PPH_TRY(la_reduce_device(ctx, sRZn, 1));
    la_p_update_dev(ctx, s.p, s.z, sRZn, sRZc, n);                          // p = z + (r.z_new / r.z) p
    return PPH_OK;
  }
  // `rotate`: r.z (current) := r.z (new) rides on the final reduction of p.Ap - after the direction update read both,
  // before the CG update reads the current one.  `want_z0`: the update also writes the next cycle's first guess into z
  int product(bool rotate, bool publish, bool want_z0) {
    published = false;
    z_ready = want_z0;
    double* z0 = want_z0 ? s.z : nullptr;
    if (merged) {
      la_spmv_dot3(ctx, *s.A, s.p, s.r, s.q, sE, rotate ? sRZn : -1, sRZc);
      PPH_TRY(la_reduce_device(ctx, sE, 4));
      la_cg_update_dev(ctx, s.x, s.r, s.p, s.q, sRZc, sE, n, sE + 3, sg, z0, pre.dinv, pre.w);   // (its r.r: local, summed with the next product's)
      return PPH_OK;
    }
    la_spmv_dot(ctx, *s.A, s.p, s.q, sPQ, rotate ? sRZn : -1, sRZc, host_tests);   // (its final reduction: inside the update kernel)
    PPH_TRY(la_reduce_device(ctx, sPQ, 1));
    // x += alpha p ; r -= alpha q ; r.r (and the next cycle's pre-smoothed first guess into z)
    published = la_cg_update_dev(ctx, s.x, s.r, s.p, s.q, sRZc, sPQ, n, sRR, sg, z0, pre.dinv, pre.w, host_tests ? -1 : S_BAD,
                                 publish ? sPQ : -1, publish ? 2 : 0);
    PPH_TRY(la_reduce_device(ctx, sRR, 1));
    return PPH_OK;
  }
  int tested_loop(const KspStop& stop, CgMemo* memo, bool x0_ready, double tol, KspOut* out);
};

// the tested loop on device scalars; out->res holds the first residual norm, `tol` what it has to reach
int CgDevice::tested_loop(const KspStop& stop, CgMemo* memo, bool x0_ready, double tol, KspOut* out) {
  double res = out->res;
  PPH_TRY(first_direction(x0_ready));
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
    gk.p[0] = s.A->ell.val ? (const void*)s.A->ell.val : (const void*)s.A->val; gk.p[1] = s.x; gk.p[2] = s.r; gk.p[3] = s.z; gk.p[4] = s.p;
    gk.p[5] = s.q; gk.p[6] = pre.dinv; gk.p[7] = pre.w;
    gk.n = n; gk.slot = s.slot; gk.epoch = ctx->mg_epoch; gk.tag = pre.tag;
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
    bool last = k + 1 >= stop.max_it;
    if (!last && guesses < 2) {
      last = (ctx->presmooth_lazy == 2) ? (memo->its == k + 1) : (memo->rho >= 0.0 && res * memo->rho <= tol);
      guesses += last ? 1 : 0;
    }
    if (last) ctx->n_presmooth_skipped++;
    return !last;
  };
  int its = 0;
  double rr_prev = res * res;   // (merged all-reduce) r.r the recurrence starts from: host-known before the first update
  while (its < stop.max_it) {
    const double res_before = res;
    if (its == 0) {
      PPH_TRY(product(false, true, want_z0(0)));
      if (merged) PPH_TRY(la_fetch_raw(ctx, sRZc, 5));   // r.z (current), p.Ap, r.Ap, Ap.Ap, r.r of the previous update
      else if (published) PPH_TRY(la_wait_published(ctx));
      else PPH_TRY(la_fetch_raw(ctx, sPQ, 2));
    } else {
      auto body = [&]() -> int {
        PPH_TRY(direction());
        PPH_TRY(product(true, true, want_z0(its)));
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
    if (stop.hist && its < stop.hist_cap) stop.hist[its] = res;
    if (!(pq > 0.0) || !(res == res)) { out->breakdown = true; break; }
    if (res <= tol) { out->converged = true; break; }
  }
  if (z_ready) ctx->n_presmooth_unused++;   // (the last update's z0: no cycle follows)
  if (memo) memo->its = its;
  out->its = its;
  out->res = res;
  return PPH_OK;
}

// the tested loop with alpha and beta on the host (a transport without device scalars)
static int cg_natural_host(pph_ctx* ctx, const CgSystem& s, const KspStop& stop, Seg sg, double tol, KspOut* out) {
  const Csr& A = *s.A;
  const int64_t n = A.nrows;
  const int slot = s.slot;
  double res = out->res;
  apply_pc(ctx, s.dinv, s.pc, s.r, s.z, n);
  la_mdot_seg(ctx, s.r, 0, 1, s.z, sg, slot);
  PPH_TRY(la_fetch(ctx, slot, 1));
  double rz = ctx->h_scal[slot];
  la_copy(ctx, s.p, s.z, n);
  int its = 0;
  while (its < stop.max_it) {
    la_spmv_dot(ctx, A, s.p, s.q, slot);
    PPH_TRY(la_fetch(ctx, slot, 1));
    const double pq = ctx->h_scal[slot];
    if (!(pq > 0.0) || !(rz == rz)) { out->breakdown = true; break; }
    const double alpha = rz / pq;
    la_cg_update(ctx, s.x, s.r, nullptr, s.p, s.q, nullptr, alpha, n, slot, sg);   // x += alpha p ; r -= alpha q ; r.r
    PPH_TRY(la_fetch(ctx, slot, 1));
    res = std::sqrt(ctx->h_scal[slot]);
    ++its;
    if (stop.hist && its < stop.hist_cap) stop.hist[its] = res;
    if (!(res == res)) { out->breakdown = true; break; }
    if (res <= tol) { out->converged = true; break; }
    apply_pc(ctx, s.dinv, s.pc, s.r, s.z, n);
    la_mdot_seg(ctx, s.r, 0, 1, s.z, sg, slot);
    PPH_TRY(la_fetch(ctx, slot, 1));
    const double rz_new = ctx->h_scal[slot];
    la_axpby(ctx, s.p, 1.0, s.z, rz_new / rz, n);
    rz = rz_new;
  }
  out->its = its;
  out->res = res;
  return PPH_OK;
}

// ------------------------------------------------------------------------------------------------
// preconditioned CG that tests the UNPRECONDITIONED residual ||r||_2 (KSP_NORM_UNPRECONDITIONED): the
// recurrence residual is known before the preconditioner is applied, so a solve of k iterations costs k
// preconditioner applications instead of k + 1 and a warm start that already meets the tolerance costs
// none.  Tolerance: max(rtol * ||b||_2, atol, reduction * ||r_0||_2).  `bnorm_hint` is ||b||_2 of an
// earlier, nearby system (see cg_start).
// ------------------------------------------------------------------------------------------------
static int cg_solve_natural(pph_ctx* ctx, const CgSystem& s, const CgStart& st, const KspStop& stop, const MgPre& pre,
                            CgMemo* memo, KspOut* out) {
  const Seg sg = pph_owned_seg(s.A->geom, s.A->nrows);
  double bnorm;
  PPH_TRY(cg_start(ctx, s, st, sg, 1, &bnorm));
  double res;
  if (st.rnorm_hint >= 0.0 && st.resumes()) {
    res = st.rnorm_hint;   // the caller knows ||r_init|| (Picard bookkeeping): no reduction, no host round trip
  } else {
    la_mdot_seg(ctx, s.r, 0, 1, s.r, sg, s.slot);
    PPH_TRY(la_fetch(ctx, s.slot, 1));
    res = std::sqrt(ctx->h_scal[s.slot]);
  }
  if (bnorm < 0.0) bnorm = res;
  const double tol = std::fmax(std::fmax(stop.rtol * bnorm, stop.atol), stop.reduction > 0.0 ? stop.reduction * res : 0.0);
  out->its = 0; out->res = res; out->converged = false; out->breakdown = false; out->bnorm = bnorm;
  if (stop.hist && stop.hist_cap > 0) stop.hist[0] = res;
  if (!(res == res)) { out->breakdown = true; return PPH_OK; }
  if (res <= tol) { out->converged = true; return PPH_OK; }
  if (!la_device_scalars(ctx)) return cg_natural_host(ctx, s, stop, sg, tol, out);
  return CgDevice(ctx, s, pre, sg, true).tested_loop(stop, memo, st.first_x0_ready && st.resumes() && pre.on, tol, out);
}

// ------------------------------------------------------------------------------------------------
// preconditioned CG without a convergence test (PETSc: ksp_norm_type none + ksp_max_it): exactly `its` iterations,
// every scalar stays on the device, NO host decision inside - a block solve is a pure launch sequence, so a whole
// Picard sweep can be enqueued (and replayed from a graph) without the GPU ever waiting for the host.  No
// preconditioner application after the last update.  Needs the device-scalar branch (la_device_scalars).
// ------------------------------------------------------------------------------------------------
static int cg_solve_fixed(pph_ctx* ctx, const CgSystem& s, const CgStart& st, int its, const MgPre& pre, KspOut* out) {
  const Seg sg = pph_owned_seg(s.A->geom, s.A->nrows);
  double bnorm;
  PPH_TRY(cg_start(ctx, s, st, sg, 2, &bnorm));
  CgDevice dev(ctx, s, pre, sg, false);
  PPH_TRY(dev.first_direction(st.first_x0_ready && st.resumes() && pre.on));
  for (int it = 0; it < its; ++it) {
    if (it > 0) PPH_TRY(dev.direction());
    PPH_TRY(dev.product(it > 0, false, pre.on && it < its - 1));   // z0 for every cycle that follows: all but the last update
  }
  // (a breakdown - p.Ap zero or NaN - is counted in scal[S_BAD] by the update kernel; the Picard loop publishes the count
  // with the sweep's norms and reports it as inner_failed)
  out->its = its; out->res = -1.0; out->converged = true; out->breakdown = false; out->bnorm = -1.0;
  return PPH_OK;
}

// preconditioned CG that tests the preconditioned residual ||z||_2 = ||P^-1 r||_2 (PETSc's default), scalars on the host
static int cg_solve_precond(pph_ctx* ctx, const CgSystem& s, const CgStart& st, const KspStop& stop, KspOut* out) {
  const Csr& A = *s.A;
  const int64_t n = A.nrows;
  const int slot = s.slot;
  // reductions run over the owned entries of a slab (whole vector on a single GPU)
  const Seg sg = pph_owned_seg(A.geom, n);
  const bool fused = (s.dinv != nullptr) || !(s.pc && *s.pc);
  double bnorm;
  PPH_TRY(cg_start(ctx, s, st, sg, 0, &bnorm));
  apply_pc(ctx, s.dinv, s.pc, s.r, s.z, n);
  la_dot2_seg(ctx, s.r, s.z, s.z, sg, slot);
  PPH_TRY(la_fetch(ctx, slot, 2));
  double rz = ctx->h_scal[slot];
  double res = std::sqrt(ctx->h_scal[slot + 1]);
  if (bnorm < 0.0) bnorm = res;
  // `reduction` > 0: also accept a drop by that factor from the initial residual of THIS solve
  const double tol = std::fmax(std::fmax(stop.rtol * bnorm, stop.atol), stop.reduction > 0.0 ? stop.reduction * res : 0.0);
  out->its = 0; out->res = res; out->converged = false; out->breakdown = false; out->bnorm = bnorm;
  if (stop.hist && stop.hist_cap > 0) stop.hist[0] = res;
  if (!(res == res)) { out->breakdown = true; return PPH_OK; }
  if (res <= tol) { out->converged = true; return PPH_OK; }
  la_copy(ctx, s.p, s.z, n);
  int its = 0;
  while (its < stop.max_it) {
    la_spmv_dot(ctx, A, s.p, s.q, slot);
    PPH_TRY(la_fetch(ctx, slot, 1));
    const double pq = ctx->h_scal[slot];
    if (!(pq > 0.0) || !(rz == rz)) { out->breakdown = true; break; }
    const double alpha = rz / pq;
    double rz_new;
    if (fused) {
      la_cg_update(ctx, s.x, s.r, s.z, s.p, s.q, s.dinv, alpha, n, slot, sg);
    } else {
      la_axpy(ctx, s.x, alpha, s.p, n);
      la_axpy(ctx, s.r, -alpha, s.q, n);
      (*s.pc)(s.r, s.z);
      la_dot2_seg(ctx, s.r, s.z, s.z, sg, slot);
    }
    PPH_TRY(la_fetch(ctx, slot, 2));
    rz_new = ctx->h_scal[slot];
    res = std::sqrt(ctx->h_scal[slot + 1]);
    ++its;
    if (stop.hist && its < stop.hist_cap) stop.hist[its] = res;
    if (!(res == res)) { out->breakdown = true; break; }
    if (res <= tol) { out->converged = true; break; }
    const double beta = rz_new / rz;
    la_axpby(ctx, s.p, 1.0, s.z, beta, n);
    rz = rz_new;
  }
  out->its = its;
  out->res = res;
  return PPH_OK;
}

// the CG driver stop.norm_type names.  `pre`, `memo`: the unpreconditioned-norm and fixed-count loops around a fused cycle
static int cg_solve(pph_ctx* ctx, const CgSystem& s, const CgStart& st, const KspStop& stop, KspOut* out,
                    const MgPre& pre = MgPre(), CgMemo* memo = nullptr) {
  if (stop.norm_type == 2 && la_device_scalars(ctx)) return cg_solve_fixed(ctx, s, st, stop.max_it, pre, out);
  if (stop.norm_type == 2) {
    // host-scalar transport: the natural-norm loop with an unreachable tolerance does the same iterations
    CgStart st2 = st;
    st2.bnorm_hint = 1.0; st2.rnorm_hint = -1.0; st2.first_x0_ready = false;
    KspStop stop2 = stop;
    stop2.rtol = 0.0; stop2.atol = 0.0; stop2.reduction = 0.0;
    const int status = cg_solve_natural(ctx, s, st2, stop2, pre, nullptr, out);
    out->converged = !out->breakdown;
    return status;
  }
  if (stop.norm_type == 1) return cg_solve_natural(ctx, s, st, stop, pre, memo, out);
  return cg_solve_precond(ctx, s, st, stop, out);
}

int pph_cg_jacobi(pph_ctx* ctx, const Csr& A, const double* b, double* x, const double* dinv, double rtol, double atol,
                  int max_it, double* r, double* z, double* p, double* q, int* its) {
  KspOut ko;
  const CgSystem sys = {.A = &A, .b = b, .x = x, .dinv = dinv, .r = r, .z = z, .p = p, .q = q, .slot = S_COARSE};
  const KspStop stop = {.rtol = rtol, .atol = atol, .max_it = max_it};
  PPH_TRY(cg_solve(ctx, sys, CgStart(), stop, &ko));
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

struct GmresSystem {   // the system of a GMRES solve (zero initial guess)
  const ApplyFn* Aop = nullptr;  // y = A x
  int64_t n = 0;
  const double* b = nullptr;
  double* x = nullptr;
  const ApplyFn* pc = nullptr;   // (none: the identity)
  int restart = 30;
  Seg sg = {0, 0, 0, 0};         // owned rows: what the reductions run over
  const GmresWs* ws = &GMRES_OUTER;
};

static int gmres_solve(pph_ctx* ctx, const GmresSystem& s, const KspStop& stop, KspOut* out) {
  const ApplyFn& Aop = *s.Aop;
  const int64_t n = s.n;
  const double* const b = s.b;
  double* const x = s.x;
  const int restart = s.restart, max_it = stop.max_it;
  const Seg sg = s.sg;
  const int S_A = s.ws->sA, S_MDOT = s.ws->sMD;   // (shadow the outer instance's slots)
  double *V, *w, *t;
  PPH_TRY(work(ctx, s.ws->idV, (size_t)(restart + 1) * (size_t)n, &V));
  PPH_TRY(work(ctx, s.ws->idW, (size_t)n, &w));
  PPH_TRY(work(ctx, s.ws->idT, (size_t)n, &t));
  std::vector<double> H((size_t)(restart + 1) * restart, 0.0), cs(restart), sn(restart), g(restart + 1), y(restart),
      hcol(restart + 2);
  auto Hat = [&](int i, int k) -> double& { return H[(size_t)k * (restart + 1) + i]; };
  la_set(ctx, x, 0.0, n);
  // r0 = P^-1 b  (zero initial guess)
  apply_pc(ctx, nullptr, s.pc, b, V, n);
  la_mdot_seg(ctx, V, 0, 1, V, sg, S_A);
  PPH_TRY(la_fetch(ctx, S_A, 1));
  double beta = std::sqrt(ctx->h_scal[S_A]);
  const double tol = std::fmax(stop.rtol * beta, stop.atol);
  out->its = 0; out->res = beta; out->converged = false; out->breakdown = false;
  if (stop.hist && stop.hist_cap > 0) stop.hist[0] = beta;
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
      apply_pc(ctx, nullptr, s.pc, t, V, n);
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
      apply_pc(ctx, nullptr, s.pc, t, w, n);
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
      if (stop.hist && its < stop.hist_cap) stop.hist[its] = res;
      if (res <= tol || its >= max_it) { done = true; break; }
    }
    // back substitution and update
    for (int i = kused - 1; i >= 0; --i) {
      double sum = g[i];
      for (int j = i + 1; j < kused; ++j) sum -= Hat(i, j) * y[j];
      y[i] = sum / Hat(i, i);
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

// where a caller that produces the residual a warm CG solve of one block starts from may leave that solve's first
// pre-smoothing z0 = dinv .* r * w (then: BlockStart::z0_ready).  z0 == nullptr: the solve has no use for it
struct PresmoothTarget {
  double* z0 = nullptr;
  const double* dinv = nullptr;
  const double* w = nullptr;          // (device)
  const SellDict* dict = nullptr;     // the block's row dictionary while usable: dinv are its 1 / a_ii
  bool ready = false;                 // z0 holds the pre-smoothing of the block's current residual
};

// what the caller of a block solve knows about its start
struct BlockStart {
  const double* r_init = nullptr;   // warm: the residual rhs - A z, known to the caller
  // vector the CG uses as its residual - on entry b - A z when warm and r_init names it, on return the recurrence
  // residual of the solve (the Picard loop keeps its block residuals there: no copies in or out)
  double* r_io = nullptr;
  double rnorm_hint = -1.0;         // >= 0: ||r_init|| over the owned rows, known to the caller
  bool z0_ready = false;            // the caller filled the block's PresmoothTarget
  bool z_is_zero = false;           // cold solve, z already zeroed
};

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
  // residual norm the block's CG ended with (unpreconditioned-norm CG only; -1 otherwise)
  double last_res = -1.0;

  int setup() {
    // ILU(0) and a Jacobi diagonal the fused assembly did not leave need CSR values (the fused assembly keeps stencil-ELL copies only)
    if (cfg->inner_pc_type == PPH_PC_ILU || (cfg->inner_pc_type == PPH_PC_JACOBI && !ctx->diag0_valid)) PPH_TRY(pph_ensure_csr_blocks(ctx));
    A[0] = block_csr(ctx, 0);
    A[1] = block_csr(ctx, 1);
    if (cfg->inner_pc_type == PPH_PC_JACOBI) {
      if (ctx->diag0_valid) {   // the fused assembly produced 1 / a_ii of both diagonal blocks
        dinv[0] = ctx->dinv0[0].p;
        dinv[1] = ctx->dinv0[1].p;
      } else {
        PPH_TRY(work(ctx, W_DINV_1, (size_t)ctx->n, &dinv[0]));
        PPH_TRY(work(ctx, W_DINV_2, (size_t)ctx->n, &dinv[1]));
        la_extract_diag_inv(ctx, A[0], dinv[0]);
        la_extract_diag_inv(ctx, A[1], dinv[1]);
      }
    } else if (cfg->inner_pc_type == PPH_PC_MG || cfg->inner_pc_type == PPH_PC_PMG) {
      // (PPH_PC_PMG reaches this point on degree-2 contexts only: mg_setup puts their operator on top of the CG-1 hierarchy)
      PPH_TRY(mg_setup(ctx));
    } else if (cfg->inner_pc_type == PPH_PC_ILU) {
      // ILU(0) of both diagonal blocks
      for (int f = 0; f < 2; ++f)
        if (!ctx->ilu[1 + f].valid) PPH_TRY(ilu_factor(ctx, ctx->ilu[1 + f], A[f]));
    } else if (cfg->inner_pc_type != PPH_PC_NONE) {
      pph_set_error(ctx, "inner pc_type %d not supported for block solves (none, jacobi, mg, pph_pmg, ilu)", cfg->inner_pc_type);
      return PPH_ERR_INVALID;
    }
    return PPH_OK;
  }

  PresmoothTarget presmooth_target(int which) {
    PresmoothTarget t;
    if (cfg->inner_ksp_type != PPH_KSP_CG || cfg->inner_pc_type != PPH_PC_MG || cfg->inner_norm == 0 || !A[which].ell.val) return t;
    const int ns = cfg->mg_smooth > 0 ? cfg->mg_smooth : 2;
    bool lo = false;
    if (!mg_pre_smoother(ctx, which, ns, &t.dinv, &t.w, &lo, &t.dict)) return PresmoothTarget();
    if (work(ctx, W_IP, (size_t)ctx->n, &t.z0) != PPH_OK) return PresmoothTarget();
    return t;
  }

  // the reference's LU block on a plumbing-size mesh (16 x 16: 289 rows): the whole block solve inside one workgroup,
  // Jacobi-CG to inner_rtol on chip - one launch instead of ~9 host-driven multigrid-CG iterations of ~10 launches and
  // one round trip each (BASELINE config 1 through solve_dpp: 20 -> ~2 ms)
  // How each of these solves ended is not looked at here (that would be the round trip this path exists to avoid): the
  // kernel adds to ctx->onchip_rec, which pph_solve_device reads once, after its final synchronisation.  A solve that
  // stops short is REPORTED (inner_failed), not repeated on the host-driven loop.
  int solve_onchip(int which, const double* rhs, double* z, double* r, double* p, double* q) {
    const int64_t n = ctx->n;
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

  // restarted GMRES on the block (FIELDSPLIT_GMRES*_PARAMS); a warm start solves for the correction (into zz)
  int solve_gmres(int which, const double* rhs, double* z, bool warm, const ApplyFn& pc, double* zz) {
    const int64_t n = ctx->n;
    const Csr& Ab = A[which];
    ApplyFn Aop = [this, &Ab](const double* xx, double* yy) { la_spmv(ctx, Ab, xx, yy); };
    ApplyFn pcj = pc;
    if (dinv[which]) { const double* dj = dinv[which]; pcj = [this, dj, n](const double* in, double* o) { la_pointwise_mult(ctx, o, dj, in, n); }; }
    GmresSystem sys = {.Aop = &Aop, .n = n, .b = rhs, .x = z, .pc = &pcj, .restart = 30, .sg = pph_owned_seg(Ab.geom, n),
                       .ws = &GMRES_INNER};
    const KspStop stop = {.rtol = cfg->inner_rtol, .atol = cfg->inner_atol, .max_it = cfg->inner_max_it};
    KspOut ko;
    if (!warm) {
      PPH_TRY(gmres_solve(ctx, sys, stop, &ko));
    } else {
      double* rr;
      PPH_TRY(work(ctx, W_IGR, (size_t)n, &rr));
      la_spmv_resid(ctx, Ab, z, rhs, rr);
      sys.b = rr; sys.x = zz;
      PPH_TRY(gmres_solve(ctx, sys, stop, &ko));
      la_axpy(ctx, z, 1.0, zz, n);
    }
    last_resid = nullptr;
    total_its += ko.its;
    if (ko.breakdown || !ko.converged) failed = true;
    return PPH_OK;
  }

  int solve(int which, const double* rhs, double* z, bool warm, const BlockStart& st = BlockStart()) {
    last_res = -1.0;
    const int64_t n = ctx->n;
    double *r, *zz, *p, *q;
    PPH_TRY(work(ctx, W_IR, (size_t)n, &r));
    if (st.r_io) r = st.r_io;
    PPH_TRY(work(ctx, W_IZ, (size_t)n, &zz));
    PPH_TRY(work(ctx, W_IP, (size_t)n, &p));
    PPH_TRY(work(ctx, W_IQ, (size_t)n, &q));
    ApplyFn pc;
    const int ns = cfg->mg_smooth > 0 ? cfg->mg_smooth : 2;
    if (cfg->inner_pc_type == PPH_PC_MG || cfg->inner_pc_type == PPH_PC_PMG)
      pc = [this, which, ns](const double* in, double* o) { mg_vcycle(ctx, which, in, o, ns); };
    if (cfg->inner_pc_type == PPH_PC_ILU)
      pc = [this, which](const double* in, double* o) { if (ilu_apply(ctx, ctx->ilu[1 + which], in, o) < 0) failed = true; };
    if (cfg->inner_exact && !cfg->picard && ctx->world == 1 && n <= 4096 && A[which].ell.val && ctx->diag0_valid && !warm)
      return solve_onchip(which, rhs, z, r, p, q);
    if (cfg->inner_ksp_type == PPH_KSP_PREONLY) {
      // one application of the inner preconditioner
      apply_pc(ctx, dinv[which], &pc, rhs, z, n);
      return PPH_OK;
    }
    if (cfg->inner_ksp_type == PPH_KSP_GMRES) return solve_gmres(which, rhs, z, warm, pc, zz);
    MgPre pre;
    if (cfg->inner_pc_type == PPH_PC_MG) pre.on = mg_pre_smoother(ctx, which, ns, &pre.dinv, &pre.w, &pre.launch_only);
    pre.tag = 16 * ns + which;
    const CgSystem sys = {.A = &A[which], .b = rhs, .x = z, .dinv = dinv[which], .pc = &pc, .r = r, .z = zz, .p = p, .q = q,
                          .slot = S_INNER};
    const CgStart start = {.warm = warm, .r_init = st.r_init, .rnorm_hint = st.rnorm_hint, .bnorm_hint = bnorm_cache[which],
                           .x_is_zero = st.z_is_zero, .first_x0_ready = st.z0_ready};
    const KspStop stop = {.rtol = cfg->inner_rtol, .atol = cfg->inner_atol, .reduction = cfg->inner_reduction,
                          .max_it = cfg->inner_max_it, .norm_type = cfg->inner_norm};
    KspOut ko;
    PPH_TRY(cg_solve(ctx, sys, start, stop, &ko, pre, &memo[which]));
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

// checks, the counters of a solve back at zero, ||rhs||
static int solve_begin(pph_ctx* ctx, const pph_solver_cfg* cfg, pph_solve_info* inf) {
  PPH_REQUIRE(ctx, ctx->asm_ok, "pph_solve before pph_assemble_dpp");
  PPH_TRY(validate_cfg(ctx, cfg));
  PPH_HIP(ctx, hipSetDevice(ctx->device));
  la_reset_spmv_stats(ctx);
  ctx->n_halo = 0;
  ctx->n_allreduce = 0;
  ctx->n_split = 0;
  if (ctx->comm_status != PPH_OK) { ctx->err = ctx->comm_error; return ctx->comm_status; }
  PPH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  inf->iterations = 0; inf->inner_iterations = 0; inf->converged = 0; inf->inner_failed = 0; inf->resnorm = 0; inf->rhs_norm = 0;
  ctx->coarse_failed = 0;
  ctx->onchip_solves = ctx->onchip_unconverged = ctx->onchip_its = 0;
  ctx->n_presmooth_skipped = ctx->n_presmooth_late = ctx->n_presmooth_unused = 0;
  la_dot(ctx, ctx->rhs.p, ctx->rhs.p, 2 * ctx->n, S_A);
  PPH_TRY(la_fetch(ctx, S_A, 1));
  inf->rhs_norm = std::sqrt(ctx->h_scal[S_A]);
  return PPH_OK;
}

// block Picard / fixed-stress sweeps on the correction du (homogeneous BCs):
//   A11 du1 = b1 - A12 du2_old ;  A22 du2 = b2 - A21 du1_new        (dpp.py:196-203)
// Residual bookkeeping: R0 = b1 - A11 du1 - A12 du2 and R1 = b2 - A21 du1 - A22 du2 are carried along.
// A block solve leaves its CG recurrence residual; when the other block moves, the residual changes by
// the change of the coupling term, which the sweep computes anyway (t12 = A12 du2, rhs1 = b2 - A21 du1).
// So a sweep costs two coupling SpMVs, the warm-started solves start from a known residual, and
// ||(R0, R1)|| is the monolithic residual (confirmed once with a true residual at convergence).
struct PicardSweeps {
  pph_ctx* ctx;
  const pph_solver_cfg* cfg;
  BlockSolver& bs;
  int64_t n = 0, pob = 0, pon = 0;   // rows of a block; the owned ones: first, count
  Csr A12, A21;
  const double *b1 = nullptr, *b2 = nullptr;
  double *du1 = nullptr, *du2 = nullptr, *pb = nullptr, *t12 = nullptr, *tn = nullptr, *rhs1 = nullptr, *R0 = nullptr, *R1 = nullptr;
  const double* rhs0 = nullptr;   // right-hand side handed to the macro block's solves
  bool recur = false;             // CG blocks: the residuals are carried along
  PresmoothTarget pt[2];          // the coupling products also write the first pre-smoothing of the block solve that follows them (fused cycle)
  double res = 0.0;               // ||(R0, R1)||
  double rn0 = -1.0;              // ||R0|| at the start of a warm sweep

  PicardSweeps(pph_ctx* c, const pph_solver_cfg* g, BlockSolver& b) : ctx(c), cfg(g), bs(b) {}

  int setup(double* du) {
    n = ctx->n;
    A12 = block_csr(ctx, 2);
    A21 = block_csr(ctx, 3);
    PPH_TRY(bs.setup());
    PPH_TRY(work(ctx, W_PB, (size_t)n, &pb));
    b1 = ctx->rhs.p;
    b2 = ctx->rhs.p + n;
    du1 = du;
    du2 = du + n;
    la_set(ctx, du, 0.0, 2 * n);
    PPH_TRY(work(ctx, W_T12, (size_t)n, &t12));
    PPH_TRY(work(ctx, W_TN, (size_t)n, &tn));
    PPH_TRY(work(ctx, W_RHS1, (size_t)n, &rhs1));
    PPH_TRY(work(ctx, W_R1, (size_t)n, &R0));
    PPH_TRY(work(ctx, W_R2, (size_t)n, &R1));
    la_set(ctx, t12, 0.0, n);
    la_set(ctx, ctx->scal.p + S_BAD, 0.0, 1);
    recur = (cfg->inner_ksp_type == PPH_KSP_CG);
    pob = ctx->mesh.own_begin();
    pon = ctx->mesh.own_end() - ctx->mesh.own_begin();
    rhs0 = pb;
    if (recur && A12.ell.val && A21.ell.val)
      for (int f = 0; f < 2; ++f) pt[f] = bs.presmooth_target(f);
    return PPH_OK;
  }

  // true residual from direct products only: t12 = A12 du2 and rhs1 = b2 - A21 du1 were formed by SpMVs with
  // the current iterates in this sweep, so two more products (A11 du1, A22 du2) complete it
  int true_residual() {
    la_sub(ctx, pb, b1, t12, n);
    rhs0 = pb;
    la_spmv_resid(ctx, bs.A[0], du1, pb, R0);
    la_spmv_resid(ctx, bs.A[1], du2, rhs1, R1);
    la_dot(ctx, R0 + pob, R0 + pob, pon, S_A);
    la_dot(ctx, R1 + pob, R1 + pob, pon, S_A + 1);
    PPH_TRY(la_fetch(ctx, S_A, 2));
    res = std::sqrt(ctx->h_scal[S_A] + ctx->h_scal[S_A + 1]);
    return PPH_OK;
  }

  // new rhs of the micro block rhs1 = b2 - A21 du1, R1 += rhs1_new - rhs1_old, ||R1||^2 -> S_B - one pass
  void couple_21() {
    la_spmv_shift(ctx, A21, du1, b2, R1, rhs1, tn, S_B, pob, pob + pon, pt[1].z0, pt[1].dinv, pt[1].w, pt[1].dict);
    pt[1].ready = pt[1].z0 != nullptr;
  }
  // new coupling term t12 = A12 du2, R0 += A12 du2_old - A12 du2_new, ||R0||^2 -> S_A - one pass (the first sweep: t12 = 0)
  void couple_12() {
    la_spmv_shift(ctx, A12, du2, nullptr, R0, t12, tn, S_A, pob, pob + pon, pt[0].z0, pt[0].dinv, pt[0].w, pt[0].dict);
    pt[0].ready = pt[0].z0 != nullptr;   // (read by the next sweep's first solve)
  }

  // Block solves without a convergence test (inner_norm 2) make a warm sweep a pure launch sequence - block solve,
  // coupling product, residual bookkeeping, block solve, coupling product, the two norms, their publication:
  // identical from sweep to sweep, so it is captured once and replayed (single context), and the only host
  // decision per sweep is the outer convergence test.
  bool launch_only() const {
    return recur && cfg->inner_norm == 2 && cfg->inner_pc_type != PPH_PC_ILU && la_device_scalars(ctx) && ctx->world == 1 &&
           ctx->fetch_spin && !ctx->time_spmv;
  }
  int enqueue_sweep() {
    // (the block solves start from the residuals R0 / R1: their right-hand sides are not read)
    PPH_TRY(bs.solve(0, pb, du1, true, {.r_init = R0, .r_io = R0, .z0_ready = pt[0].ready}));
    couple_21();
    PPH_TRY(bs.solve(1, rhs1, du2, true, {.r_init = R1, .r_io = R1, .z0_ready = pt[1].ready}));
    couple_12();
    la_dot(ctx, R1 + pob, R1 + pob, pon, S_A + 1);
    la_publish(ctx, S_A, 4);   // ||R0||^2, ||R1||^2, (S_B), breakdowns counted by the block solves (S_BAD)
    return PPH_OK;
  }
  int launch_only_sweep() {
    const int its_before = bs.total_its;
    if (ctx->use_graphs == 2) {   // (measured after the kernel work of round 2: the eager sweep is faster, 64^3 2.65 vs 2.80 ms - the host runs ahead of a launch-only sequence anyway; a replay only adds its start-up latency)
      GraphKey gk;
      gk.p[0] = du1; gk.p[1] = R0; gk.p[2] = R1; gk.p[3] = t12; gk.p[4] = tn; gk.p[5] = rhs1; gk.p[6] = pb;
      gk.p[7] = bs.A[0].ell.val ? (const void*)bs.A[0].ell.val : (const void*)bs.A[0].val;
      gk.n = n; gk.slot = cfg->inner_max_it; gk.epoch = ctx->mg_epoch;
      gk.tag = 5000 + 64 * cfg->inner_pc_type + (cfg->mg_smooth > 0 ? cfg->mg_smooth : 2);
      PPH_TRY(la_run_graph(ctx, gk, [this]() -> int { return enqueue_sweep(); }));
    } else {
      PPH_TRY(enqueue_sweep());
    }
    if (bs.total_its == its_before) bs.total_its += 2 * cfg->inner_max_it;   // a replayed sweep: counted here
    PPH_TRY(la_wait_published(ctx));
    if (ctx->h_scal[S_BAD] != 0.0) bs.failed = true;
    res = std::sqrt(ctx->h_scal[S_A] + ctx->h_scal[S_A + 1]);
    return PPH_OK;
  }

  int general_sweep(bool warm) {
    // a warm CG block solve starts from its carried residual (R0 / R1) and a cached ||b||: its right-hand side is
    // not read; with the unpreconditioned-norm test the host also knows the residual norms already (hints)
    const bool hints = warm && recur && cfg->inner_norm == 1;
    // rhs of the macro block.  Cold sweep of the CG blocks: t12 = +0, and b - (+0) == b bit for bit (-0 included), so
    // the solve reads b1 itself instead of a copy; as before, the warm sweeps are handed what the last la_sub left
    if (!warm && recur) rhs0 = b1;
    else if (!recur) la_sub(ctx, pb, b1, t12, n);
    // (cold: du was zeroed above and nothing has written the block since)
    PPH_TRY(bs.solve(0, rhs0, du1, warm, {.r_init = (warm && recur) ? R0 : nullptr, .r_io = recur ? R0 : nullptr,
                                          .rnorm_hint = hints ? rn0 : -1.0, .z0_ready = pt[0].ready, .z_is_zero = !warm}));
    double rn1 = -1.0;
    if (warm && recur) {
      couple_21();
      if (hints) {
        PPH_TRY(la_fetch(ctx, S_B, 1));
        rn1 = std::sqrt(ctx->h_scal[S_B]);
      }
    } else {
      la_spmv_resid(ctx, A21, du1, b2, rhs1);
    }
    PPH_TRY(bs.solve(1, rhs1, du2, warm, {.r_init = (warm && recur) ? R1 : nullptr, .r_io = recur ? R1 : nullptr,
                                          .rnorm_hint = rn1, .z0_ready = pt[1].ready, .z_is_zero = !warm}));
    if (!recur) {
      la_spmv(ctx, A12, du2, tn);                                  // new coupling term
      la_copy(ctx, t12, tn, n);
      return true_residual();
    }
    couple_12();
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
    return PPH_OK;
  }
};

static int solve_picard(pph_ctx* ctx, const pph_solver_cfg* cfg, BlockSolver& bs, double* du, double* hist, int hist_cap,
                        pph_solve_info* inf) {
  PicardSweeps P(ctx, cfg, bs);
  PPH_TRY(P.setup(du));
  const double r0 = inf->rhs_norm;
  const double tol = std::fmax(cfg->picard_rtol * r0, cfg->picard_atol);
  P.res = r0;
  if (hist && hist_cap > 0) hist[0] = P.res;
  int its = 0;
  const bool launch_only = P.launch_only();
  while (P.res > tol && its < cfg->picard_max_it) {
    const bool warm = its > 0;
    if (warm && launch_only) PPH_TRY(P.launch_only_sweep());
    else PPH_TRY(P.general_sweep(warm));
    ++its;
    if (hist && its < hist_cap) hist[its] = P.res;
    if (!(P.res == P.res)) break;
    if (P.res <= tol && P.recur) {
      // confirm with the true residual once; keep sweeping if the recurrences were optimistic
      PPH_TRY(P.true_residual());
      if (hist && its < hist_cap) hist[its] = P.res;
    }
  }
  inf->iterations = its;
  inf->inner_iterations = bs.total_its;
  inf->resnorm = P.res;
  inf->converged = (P.res <= tol) ? 1 : 0;
  inf->inner_failed = (bs.failed || ctx->coarse_failed) ? 1 : 0;
  return inf->converged ? PPH_OK : PPH_ERR_DIVERGED;
}

// one Krylov solve of the monolithic system
static int solve_monolithic(pph_ctx* ctx, const pph_solver_cfg* cfg, BlockSolver& bs, double* du, double* hist, int hist_cap,
                            pph_solve_info* inf) {
  const int64_t n = ctx->n, N = 2 * n;
  const Csr A21 = block_csr(ctx, 3);
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
  const KspStop stop = {.rtol = cfg->rtol, .atol = cfg->atol, .max_it = cfg->max_it, .hist = hist, .hist_cap = hist_cap};
  if (cfg->ksp_type == PPH_KSP_PREONLY) {
    apply_pc(ctx, nullptr, &pc, ctx->rhs.p, du, N);
    ko.its = 1; ko.res = 0.0; ko.converged = true;
  } else if (cfg->ksp_type == PPH_KSP_CG) {
    CgSystem sys = {.A = &A, .b = ctx->rhs.p, .x = du, .dinv = dinv, .pc = &pc, .slot = S_B};
    PPH_TRY(work(ctx, W_R, (size_t)N, &sys.r));
    PPH_TRY(work(ctx, W_Z, (size_t)N, &sys.z));
    PPH_TRY(work(ctx, W_P, (size_t)N, &sys.p));
    PPH_TRY(work(ctx, W_Q, (size_t)N, &sys.q));
    PPH_TRY(cg_solve(ctx, sys, CgStart(), stop, &ko));
  } else {
    const GmresSystem sys = {.Aop = &Aop, .n = N, .b = ctx->rhs.p, .x = du, .pc = &pc, .restart = cfg->restart,
                             .sg = pph_owned_seg(A.geom, N)};
    PPH_TRY(gmres_solve(ctx, sys, stop, &ko));
  }
  if (cfg->pc_type == PPH_PC_CMG) PPH_TRY(cmg_collect_failures(ctx));   // coarsest solves on the device that stopped short
  inf->iterations = ko.its;
  inf->inner_iterations = bs.total_its;
  inf->resnorm = ko.res;
  inf->converged = (ko.converged && !bs.failed) ? 1 : 0;
  inf->inner_failed = (bs.failed || ctx->coarse_failed) ? 1 : 0;
  return (!ko.converged || ko.breakdown) ? PPH_ERR_DIVERGED : PPH_OK;
}

// u = u0 + du, the record of the on-chip block solves, timers, what the device reported meanwhile; `status`: PPH_OK or
// PPH_ERR_DIVERGED of the solve
static int solve_finish(pph_ctx* ctx, const BlockSolver& bs, const double* du, int status, pph_solve_info& inf, pph_solve_info* info) {
  const int64_t N = 2 * ctx->n;
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

int pph_solve_device(pph_ctx* ctx, const pph_solver_cfg* cfg, pph_solve_info* info, double* hist, int hist_cap) {
  if (!ctx) return PPH_ERR_INVALID;
  pph_solve_info inf;
  PPH_TRY(solve_begin(ctx, cfg, &inf));
  // a degree-1 context has no p-level to add: there PPH_PC_PMG is PPH_PC_MG, path for path
  pph_solver_cfg cfg_mg;
  if (cfg->inner_pc_type == PPH_PC_PMG && ctx->mesh.degree == 1) {
    cfg_mg = *cfg;
    cfg_mg.inner_pc_type = PPH_PC_MG;
    cfg = &cfg_mg;
  }
  double* du;
  PPH_TRY(work(ctx, W_DU, (size_t)(2 * ctx->n), &du));
  BlockSolver bs;
  bs.ctx = ctx; bs.cfg = cfg;
  const int status = cfg->picard ? solve_picard(ctx, cfg, bs, du, hist, hist_cap, &inf)
                                 : solve_monolithic(ctx, cfg, bs, du, hist, hist_cap, &inf);
  if (status < 0 && status != PPH_ERR_DIVERGED) return status;
  return solve_finish(ctx, bs, du, status, inf, info);
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
