/*
 * perphil_hip.h — C ABI of the MI355X-native DPP hot path (libperphil_hip.so).
 *
 * The reference (ThermoPhase-FCSRG/perphil) exposes no FFI: its boundary for this path is the
 * Python call  solve_dpp(W, model_params, bcs, solver_parameters, options_prefix) -> Solution
 * (reference src/perphil/solvers/solver.py:30-76) whose arithmetic runs inside Firedrake/PETSc.
 * This header declares what a ctypes binding of that call needs; each entry point cites the
 * reference interface (or the third-party work triggered from it) that it replaces.
 * perphil_amd/_ffi.py is the binding; INTEGRATION.md shows the stub a perphil maintainer adds.
 *
 * Conventions
 *   - every function returns 0 on success, a negative pph_status on failure; no exceptions and
 *     no aborts cross this boundary; pph_last_error() returns a message for the last failure.
 *   - the caller owns every host buffer it passes (borrowed for the duration of the call only);
 *     the library owns all device memory behind the opaque handle; nothing returned by pointer
 *     outlives pph_ctx_destroy().
 *   - one host thread drives one context (not re-entrant); independent contexts are independent.
 *   - numbering: node (i,j,k) -> i + (nx+1)*(j + (ny+1)*k) inside the LOCAL box of the context;
 *     degree 2 (pph_mesh_build_lagrange): the nodes are the points of the lattice refined once, node (I,J,K) ->
 *     I + (2nx+1)*(J + (2ny+1)*K) at (I/2nx, J/2ny, K/2nz); local node order of a cell: Q2 quads / hexes the lattice
 *     offset (a,b,c) in {0,1,2}^d of the box -> a + 3b (+ 9c); P2 triangles / tetrahedra the cell's CG-1 vertices (in
 *     the CG-1 dof map's order), then the edge midpoints 01, 02, 12 / 01, 02, 03, 12, 13, 23 (perphil_amd/csrc/pph_p2.h);
 *     monolithic dof = field*n + node (field-major; reference
 *     src/perphil/experiments/iterative_bench.py:323-324).
 *   - all floating point is IEEE fp64; indices are int32 (columns, cell->dof map) / int64 (row
 *     pointers, counts).
 */
#ifndef PERPHIL_HIP_H
#define PERPHIL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pph_ctx pph_ctx;

typedef enum {
  PPH_OK = 0,
  PPH_ERR_INVALID = -1,   /* bad argument / call order          -> Python ValueError   */
  PPH_ERR_HIP = -2,       /* HIP runtime failure                -> Python RuntimeError */
  PPH_ERR_NOMEM = -3,     /* device or host allocation failed   -> Python MemoryError  */
  PPH_ERR_DIVERGED = -4,  /* Krylov/Picard hit max_it or broke down (result still written) */
  PPH_ERR_COMM = -5       /* RCCL failure                                              */
} pph_status;

/* cell kinds of the structured unit square / cube
 * (reference src/perphil/mesh/builtin.py:20 -> fd.UnitSquareMesh quads / "left"-diagonal
 *  triangles; src/perphil/experiments/petsc_profiling_3d.py:31 -> fd.UnitCubeMesh, 6 Kuhn tets
 *  per cube; notebooks/condition-number-study-3d.py:66 -> hexahedral=True) */
enum { PPH_CELL_QUAD = 0, PPH_CELL_TRI = 1, PPH_CELL_HEX = 2, PPH_CELL_TET = 3 };

/* Krylov / preconditioner / outer-loop kinds: the supported subset of the PETSc option
 * dictionaries in reference src/perphil/solvers/parameters.py:4-102 */
enum { PPH_KSP_PREONLY = 0, PPH_KSP_CG = 1, PPH_KSP_GMRES = 2 };
enum {
  PPH_PC_NONE = 0,
  PPH_PC_JACOBI = 1,      /* pc_type jacobi                                              */
  PPH_PC_BLOCK2 = 2,      /* 2x2 node-block Jacobi (both pressures of one node coupled)    */
  PPH_PC_FIELDSPLIT = 3,  /* pc_type fieldsplit, pc_fieldsplit_type multiplicative         */
  PPH_PC_MG = 4,          /* geometric multigrid V-cycle (scalar blocks; inside fieldsplit/Picard) */
  PPH_PC_ILU = 5,         /* pc_type ilu, pc_factor_levels 0: ILU(0) in the natural row order, level-scheduled
                           * (monolithic system, or the scalar blocks inside fieldsplit / Picard); single context */
  PPH_PC_PMG = 6,         /* pph_pmg (scalar blocks; inside fieldsplit / Picard, as inner_pc_type): one symmetric V-cycle whose
                           * top level is the context's own operator and whose lower levels are the CG-1 geometric hierarchy
                           * on the same cells.  Degree 2: mg_smooth Chebyshev-Jacobi steps on the Q2 / P2 operator, restriction
                           * to the CG-1 space of the same cells (the degree-2 nodes are the CG-1 nodes of the mesh refined
                           * once, so this is the h-transfer stencil), the PPH_PC_MG cycle there, and back.  Degree 1: there is
                           * no p-level to add, PPH_PC_PMG is PPH_PC_MG. */
  PPH_PC_CMG = 7          /* pph_cmg (monolithic system; pc_type of a cg / gmres / preonly solve with picard == 0): one symmetric
                           * V-cycle on the coupled 2n x 2n system over the CG-1 hierarchy of PPH_PC_MG.  Level operator
                           * A_l = [[A11_l, C_l], [C_l^T, A22_l]] with the level operators of the scalar cycle on the diagonal
                           * and C_l = -(beta/mu) F0 M_l F1 (M_l the level's mass matrix, F_f zeroes the constrained dofs of
                           * field f); smoother: mg_smooth Chebyshev steps on [lam_l / 4, lam_l] under the inverse of the 2 x 2
                           * block of the two pressures of every node (diagonal where either field is constrained), lam_l the
                           * largest absolute row sum of D_l^-1 A_l; transfers: those of PPH_PC_MG per field, each with its own
                           * masks; coarsest level: CG on A_L under D_L^-1 to rtol 1e-12, limited by option coarse_max_it (a
                           * solve that stops short is reported as inner_failed); a mesh that cannot be coarsened: max(mg_smooth,
                           * 2) Chebyshev steps.  fp64, no floating-point atomics.  Refused (PPH_ERR_INVALID with a message) as
                           * inner_pc_type, with picard, on a degree-2 context and with world != 1. */
};

typedef struct {
  int32_t ksp_type;      /* PPH_KSP_*  (ksp_type)                                        */
  int32_t pc_type;       /* PPH_PC_*   (pc_type)                                         */
  int32_t restart;       /* GMRES restart, PETSc default 30                              */
  int32_t max_it;        /* ksp_max_it                                                   */
  double rtol;           /* ksp_rtol                                                     */
  double atol;           /* ksp_atol                                                     */
  /* block solves of the field-split PC / Picard sweeps (fieldsplit_0_/fieldsplit_1_ options;
   * the reference's LU block solves become inner Krylov solves run to inner_rtol)          */
  int32_t inner_ksp_type;   /* PPH_KSP_PREONLY | PPH_KSP_CG | PPH_KSP_GMRES (restart 30, zero guess per solve) */
  int32_t inner_pc_type;    /* PPH_PC_NONE | PPH_PC_JACOBI | PPH_PC_MG | PPH_PC_ILU | PPH_PC_PMG */
  int32_t inner_max_it;
  int32_t picard;        /* 0: Krylov on the monolithic system; 1: block Picard (fixed-stress)
                          * outer loop per reference src/perphil/forms/dpp.py:196-203       */
  double inner_rtol;
  double inner_atol;
  double picard_rtol;    /* snes_rtol */
  double picard_atol;    /* snes_atol */
  int32_t picard_max_it; /* snes_max_it */
  int32_t mg_smooth;     /* smoothing steps per level side for PPH_PC_MG / PPH_PC_PMG / PPH_PC_CMG (default 2; every level,
                          * the degree-2 one included) */
  double inner_reduction; /* > 0: block solves stop once their preconditioned residual has dropped by this
                          * factor from its value at the start of the solve (inexact Picard sweeps; warm
                          * starts make the sequence converge to the exact fixed point), or at inner_rtol,
                          * whichever comes first.  0: inner_rtol only.                       */
  int32_t inner_norm;    /* norm the block solves test (ksp_norm_type of the fieldsplit_i_ solvers): 0 =
                          * preconditioned ||P^-1 r|| (PETSc's default for left-preconditioned CG), 1 =
                          * unpreconditioned ||r||_2 (KSP_NORM_UNPRECONDITIONED): the recurrence residual is
                          * known before the preconditioner runs, so a block solve of k iterations costs k
                          * preconditioner applications instead of k + 1; 2 = none (KSP_NORM_NONE): no convergence
                          * test, every block solve runs exactly inner_max_it CG iterations - a Picard sweep then
                          * holds no host decision and is enqueued (replayed from a hipGraph) in one go              */
  int32_t inner_exact;   /* 1: the block solves stand for the reference's LU blocks (fieldsplit_i_pc_type lu): where a block has at
                          * most 4096 rows (the plumbing configurations) it is solved to inner_rtol inside ONE workgroup, on chip
                          * (Jacobi-CG, no host round trip), instead of by the host-driven Krylov loop; larger blocks: as inner_*
                          * say.  0: always as inner_* say                                                              */
} pph_solver_cfg;

typedef struct {
  int32_t iterations;        /* outer Krylov its (ksp.getIterationNumber(), solver.py:73) or Picard sweeps */
  int32_t inner_iterations;  /* total inner Krylov iterations                            */
  int32_t converged;         /* 1 / 0                                                    */
  int32_t inner_failed;      /* 1: a block solve of the field-split PC / a Picard sweep, or the coarsest multigrid
                              * solve, hit its iteration limit or broke down (the outer result may still converge);
                              * also an on-chip LU-equivalent block solve that ended short of its tolerance
                              * (pph_get_timers out[26..28]) */
  double resnorm;            /* final (preconditioned) residual norm (ksp.getResidualNorm(), solver.py:74) */
  double rhs_norm;           /* ||F(u0)||_2, PETSc's "0 SNES Function norm"               */
} pph_solve_info;

/* ---- context ------------------------------------------------------------------------- */
/* replaces: process-wide PETSc/Firedrake initialisation behind `import firedrake` */
int pph_ctx_create(int device, pph_ctx** out);
int pph_ctx_destroy(pph_ctx* ctx);
/* message of the last failure on ctx (ctx may be NULL: last failure of pph_ctx_create) */
const char* pph_last_error(const pph_ctx* ctx);
/* blocks until all device work of the context has finished */
int pph_ctx_synchronize(pph_ctx* ctx);

/* ---- mesh + cell->dof map --------------------------------------------------------------
 * replaces: create_mesh() (reference src/perphil/mesh/builtin.py:4-20), fd.UnitCubeMesh call
 * sites (petsc_profiling_3d.py:31), create_function_spaces()/MixedFunctionSpace (CG-1 dof map,
 * src/perphil/forms/spaces.py:34-35).
 * The context's LOCAL box holds cell layers [z_cell_begin, z_cell_begin+z_cell_count) of the
 * global nx*ny*nz mesh (2D: nz = 0, z_cell_begin = 0, z_cell_count = 0).  ghost_lo / ghost_hi
 * mark the lowest / highest local node plane as a ghost plane owned by the neighbouring slab
 * (multi-GPU cell-slab decomposition); single GPU: whole mesh, no ghosts. */
int pph_mesh_build(pph_ctx* ctx, int dim, int cell_kind, int nx, int ny, int nz,
                   int z_cell_begin, int z_cell_count, int ghost_lo, int ghost_hi);
/* Whole mesh (one context, no slabs) with Lagrange pressures of degree 1 or 2 (reference create_function_spaces(mesh,
 * pressure_deg=...), src/perphil/forms/spaces.py:5-36).  Degree 1 is pph_mesh_build of the whole mesh.  Degree 2: Q2 / P2
 * nodes on the refined lattice (numbering above; nodes per cell 9 / 6 / 27 / 10); every call below then works on those
 * nodes, on CSR operators (no stencil-ELL storage).  Multigrid at degree 2 is PPH_PC_PMG (block solves of a field split /
 * Picard sweep: the degree-2 operator on top of the CG-1 hierarchy of the same cells).  A cfg with pc_type mg, or whose
 * field-split / Picard block solves use PPH_PC_MG, returns PPH_ERR_INVALID with a message, and so does
 * pph_darcy_velocity*. */
int pph_mesh_build_lagrange(pph_ctx* ctx, int dim, int cell_kind, int nx, int ny, int nz, int degree);
int pph_mesh_sizes(const pph_ctx* ctx, int64_t* n_nodes, int64_t* n_cells, int32_t* nodes_per_cell,
                   int64_t* nnz_block);
int pph_get_dofmap(pph_ctx* ctx, int32_t* cells_host /* [n_cells][nodes_per_cell] */);
int pph_get_coords(pph_ctx* ctx, double* coords_host /* [n_nodes][dim] */);

/* ---- Dirichlet data ---------------------------------------------------------------------
 * replaces: fd.DirichletBC(W.sub(field), expr, "on_boundary") as consumed at
 * reference src/perphil/solvers/solver.py:66.  `nodes` are local node ids, `vals` the boundary
 * values (evaluated by the caller, e.g. from the manufactured solution,
 * src/perphil/utils/manufactured_solutions.py:39-51,87-88).  Replaces earlier data of `field`. */
int pph_set_dirichlet(pph_ctx* ctx, int field, const int64_t* nodes, const double* vals, int64_t count);
/* the same from DEVICE arrays (nodes, vals: `count` entries in memory of the context's device, e.g. torch tensors): the
 * node range is checked on the device, then the mask / value scatter of pph_set_dirichlet runs on the context stream.
 * Returns once the context stream has finished with both arrays. */
int pph_set_dirichlet_device(pph_ctx* ctx, int field, const int64_t* nodes, const double* vals, int64_t count);

/* ---- assembly -----------------------------------------------------------------------------
 * replaces: dpp_form() (reference src/perphil/forms/dpp.py:95-132) + the TSFC element kernel /
 * PyOP2 cell loop / MatSetValues / BC elimination that solver.solve() triggers
 * (src/perphil/solvers/solver.py:71 -> SNESJacobianEval), and dpp_delayed_form() (dpp.py:135-205).
 * Builds on device: scalar CSR pattern, K and M by cell-local integration + scatter-add, then the
 * Dirichlet-eliminated blocks A11 = (k1/mu)K + (beta/mu)M, A22 = (k2/mu)K + (beta/mu)M,
 * A12 = A21^T = -(beta/mu)M and the lifted right-hand side.  `monolithic != 0` additionally
 * materialises the 2n x 2n field-major CSR. */
int pph_assemble_dpp(pph_ctx* ctx, double k1, double k2, double beta, double mu, int monolithic);
/* The same system with PER-FIELD mass coefficients (no reference counterpart; the operator of a theta time step, below):
 *   A11 = (k1/mu) K + (beta/mu + sigma1) M,   A22 = (k2/mu) K + (beta/mu + sigma2) M,   A12 = A21^T = -(beta/mu) M,
 * Dirichlet-eliminated as above, lifted right-hand side -F A_shifted,unel u0.  sigma_f must be finite and >= 0 (PPH_ERR_INVALID
 * with a message otherwise); sigma = (0, 0) IS pph_assemble_dpp: the same kernels, the same bits.  With a sigma != 0: single
 * context only; the fused assembly takes the tile / two-pass kernels (the node kernel forms one mass coefficient for the three
 * blocks), the shift's share -sigma_f F M g_f of the lifting is one matrix-free product behind the fused kernels (inside the
 * two-step path's own lifting kernel otherwise), and every level of the multigrid hierarchies (PPH_PC_MG, PPH_PC_PMG,
 * PPH_PC_CMG: d_ff = coefK_f K_ii + (beta/mu + sigma_f) M_ii, coupling -(beta/mu) M) is built with the coefficients of its
 * field.  Every assembly invalidates hierarchies and factorisations: a change of sigma is a new system. */
int pph_assemble_dpp_shifted(pph_ctx* ctx, double k1, double k2, double beta, double mu, double sigma1, double sigma2,
                             int monolithic);

/* ---- solve --------------------------------------------------------------------------------
 * replaces: LinearVariationalSolver.solve() -> KSPSolve (reference src/perphil/solvers/solver.py:67-71);
 * with cfg->picard the block Picard loop stated by dpp_delayed_form (dpp.py:196-203).
 * x_host (len 2n, caller-owned) receives the full solution u = u0 + du, field-major.
 * hist (optional, capacity hist_cap) receives residual norms per outer iteration, entry 0 = initial. */
int pph_solve(pph_ctx* ctx, const pph_solver_cfg* cfg, double* x_host, pph_solve_info* info,
              double* hist, int hist_cap);
/* same solve, result left on the device (timing without the PCIe copy); fetch with pph_get_solution */
int pph_solve_device(pph_ctx* ctx, const pph_solver_cfg* cfg, pph_solve_info* info, double* hist, int hist_cap);
int pph_get_solution(pph_ctx* ctx, double* x_host /* len 2n */);
/* Device-resident results (no reference counterpart: Firedrake's Function lives in host memory).  The context's HIP stream
 * (a hipStream_t, non-blocking) for ordering a caller's own device work against the library's in both directions; and a copy
 * of the current solution (field-major, count = 2n local) into a CALLER-OWNED device buffer, enqueued on that stream and not
 * waited for.  The library never frees nor keeps dst. */
int pph_get_stream(pph_ctx* ctx, void** stream);
int pph_copy_solution_device(pph_ctx* ctx, double* dst, int64_t count);
/* Page-locked host memory for the x_host / result arrays above (no reference counterpart: PETSc's Vec lives in host memory
 * already).  A copy into pageable memory is staged by the HIP runtime and pays the first touch of a fresh array's pages; the
 * Python host side keeps a small pool of pinned result buffers (perphil_amd/_ffi.py: Context.solution).  Freed with
 * pph_host_free; both are independent of any context. */
int pph_host_alloc(size_t bytes, void** out);
int pph_host_free(void* p);

/* ---- export for parity checks -----------------------------------------------------------
 * replaces: get_matrix_data_from_form() -> petsc_matrix.getValuesCSR()
 * (reference src/perphil/solvers/conditioning.py:66-102).
 * which: 0 monolithic (needs monolithic assembly), 1 K, 2 M, 3 A11, 4 A22, 5 A12, 6 A21 */
int pph_csr_sizes(const pph_ctx* ctx, int which, int64_t* nrows, int64_t* nnz);
int pph_get_csr(pph_ctx* ctx, int which, int64_t* rowptr, int32_t* col, double* val);
int pph_get_rhs(pph_ctx* ctx, double* rhs_host /* len 2n */, double* u0_host /* len 2n, may be NULL */);
/* y = A x with the selected matrix (host vectors); replaces PETSc MatMult for tests */
int pph_spmv(pph_ctx* ctx, int which, const double* x_host, double* y_host);
/* `reps` back-to-back device SpMVs on resident vectors, average kernel ms via HIP events */
int pph_spmv_bench(pph_ctx* ctx, int which, int reps, double* avg_ms);
/* z = B r: ONE application of a block preconditioner of the assembled system to a host vector (no reference counterpart:
 * PETSc's PCApply; here for parity checks of a cycle itself rather than of its fixed point).  which: 0 the A11 block, 1 the
 * A22 block (length n each).  pc_type: PPH_PC_JACOBI | PPH_PC_MG | PPH_PC_PMG | PPH_PC_ILU; mg_smooth as in pph_solver_cfg
 * (<= 0: 2).  The entries of r on constrained dofs are taken as 0, as the residuals of the Krylov loops are; the result is 0
 * there.  PPH_PC_MG on a degree-2 context returns PPH_ERR_INVALID, PPH_PC_PMG on a degree-1 context is PPH_PC_MG.  Single
 * context only. */
int pph_pc_apply(pph_ctx* ctx, int which, int pc_type, int mg_smooth, const double* r_host, double* z_host);
/* z = B r: ONE application of a preconditioner of the monolithic system to a host vector of 2n entries (field-major), for
 * parity checks of the coupled cycle itself.  pc_type: PPH_PC_CMG | PPH_PC_BLOCK2 | PPH_PC_JACOBI; mg_smooth as in
 * pph_solver_cfg (<= 0: 2).  Needs the monolithic assembly.  The entries of r on constrained dofs are taken as 0; the
 * result is 0 there.  Single context, degree 1 for PPH_PC_CMG. */
int pph_pc_apply_coupled(pph_ctx* ctx, int pc_type, int mg_smooth, const double* r_host /* 2n */, double* z_host /* 2n */);
/* diagnostic (tools/cmg_probe.py): `reps` PPH_PC_CMG cycles on a device-resident vector of ones and `reps` fine-level
 * passes of the coupled smoothing kernel alone, timed with HIP events.  out4: ms per cycle; ms per such pass; its
 * algorithmic bytes; ms of set-up the call had to do first */
int pph_cmg_bench(pph_ctx* ctx, int mg_smooth, int reps, double* out4);
/* diagnostic (tools/pmg_probe.py): `reps` applications to a device-resident vector of ones, timed with HIP events.
 * out4: ms per application; ms of it in the passes over the degree-2 level (PPH_PC_PMG at degree 2, else 0); bytes those
 * passes move per application (the kernels of pph_pmg.hip, else 0); ms of set-up the call had to do first */
int pph_pc_bench(pph_ctx* ctx, int which, int pc_type, int mg_smooth, int reps, double* out4);

/* HBM bandwidth calibration on this device (tools/bw_probe.py, tools/pmc_probe.py): `bytes` streamed with
 * 16 B per lane by `blocks` workgroups, mode 0 read-only, mode 1 copy; average ms per launch. */
int pph_bw_probe(pph_ctx* ctx, int64_t bytes, int mode, int blocks, double* ms_out);

/* diagnostic, host only (no device is touched): the wave map of the node assembly kernel's two launches (option
 * asm_node_lines) for a box of px x py x pz nodes (dim 2: pz = 1) with `near[row] != 0` on the rows that need the Dirichlet
 * masks (null: none); align: the option's value (1: the default alignment of a window's first row, or 2, 4 .. 64 rows).
 * win: first row of every straight-line window of 64 consecutive rows; pairs: the even row of every
 * aligned row pair of the general launch, padded to a multiple of 32 pairs.  counts[0..1] receive the two lengths; win /
 * pairs may be null (sizes only), else they hold at least that many entries. */
int pph_asm_wave_map(int dim, int px, int py, int pz, int align, const uint8_t* near, uint32_t* win, uint32_t* pairs, int64_t* counts);

/* ---- extreme eigenvalues / condition numbers on the device -------------------------------------------
 * replaces: calculate_condition_number() of the exported matrix (reference src/perphil/solvers/conditioning.py:105-218)
 * for the symmetric positive definite operators: kappa = lambda_max / lambda_min without the matrix leaving the device.
 *
 * extreme eigenvalues of a symmetric operator of the context, plain Lanczos on the device (no reorthogonalisation).
 * which: 0 monolithic (needs monolithic assembly), 2 M, 3 A11, 4 A22 (pph_get_csr's selectors; anything else,
 * or world != 1: PPH_ERR_INVALID with a message).  Works on degree-1 and degree-2 contexts; the product is the one pph_spmv
 * would run (stencil-ELL copy or row dictionary for the CG-1 blocks, CSR for the monolithic system and degree 2).
 * tol <= 0: 1e-10; max_it <= 0: 20 000; check_every <= 0: 32.  Start vector: a fixed hash of the row index, normalised.
 * Every check_every steps the host reads the recurrence coefficients (one synchronisation) and takes the extremes theta of the
 * tridiagonal matrix T they form; an end is converged when |beta_m s_m| <= tol |theta| (s_m: last component of T's normalised
 * eigenvector) and stays converged.  Breakdown: the first j with beta_j not finite or <= 1e-13 max(|alpha_i|, beta_0) ends the
 * recurrence on an invariant subspace; the extremes of T's leading j + 1 rows are then exact.
 * out[0] lambda_min, out[1] lambda_max, out[2] Lanczos steps taken, out[3] 1 converged / 0 stopped at max_it (values still
 * returned), out[4] 1 when the recurrence ended on an invariant subspace (breakdown), out[5], out[6] the final estimates
 * |beta_m s_m| of the two ends (0 after a breakdown), out[7] ms on the device (event pair), out[12] rows of the T the values
 * were taken from (= out[2], or j + 1 after a breakdown).
 * vec_lo / vec_hi: NULL, or caller-owned DEVICE arrays of nrows doubles that receive the normalised Ritz vectors (a second
 * pass of the same recurrence accumulates them; the context stream has finished with them on return); then out[8], out[9] =
 * their Rayleigh quotients, out[10], out[11] = ||A y - rq y||_2.  A plain-Lanczos Ritz vector's residual is NOT bounded by
 * tol: it is reported, not promised.
 * fp64, no floating-point atomics: two calls give the same bits.  Memory: 3 vectors of nrows (5 with Ritz vectors) and
 * 2 max_it doubles, released on return. */
int pph_extreme_eigenvalues(pph_ctx* ctx, int which, double tol, int max_it, int check_every,
                            double* vec_lo, double* vec_hi, double* out /* [13], host */);
/* extreme eigenvalues of the PRECONDITIONED operator B A: what a Krylov method under one of the library's symmetric
 * preconditioners sees (kappa(B A) = out[1] / out[0]), without A or B leaving the device (no reference counterpart: the
 * reference's studies stop at the unpreconditioned operators).  Lanczos for the pencil (A, B^-1) in the B inner product: two
 * sequences u_j and v_j = B u_j, one product and one preconditioner application per step, B^-1 never applied, no
 * reorthogonalisation.
 * which / pc_type (everything else, or world != 1: PPH_ERR_INVALID with a message):
 *   3 (A11), 4 (A22): PPH_PC_JACOBI, PPH_PC_ILU, PPH_PC_MG (degree-1 contexts only), PPH_PC_PMG (at degree 1 it is PPH_PC_MG);
 *   0 (monolithic, needs monolithic assembly): PPH_PC_JACOBI, PPH_PC_BLOCK2, PPH_PC_ILU, PPH_PC_CMG (degree-1 contexts);
 *   2 (M): PPH_PC_JACOBI.
 * PPH_PC_NONE is refused (that is pph_extreme_eigenvalues), PPH_PC_FIELDSPLIT as well (the multiplicative split is not
 * symmetric).  mg_smooth as in pph_solver_cfg (<= 0: 2).
 * Constrained rows: the iteration runs on the FREE rows only - the start vector (the hash of pph_extreme_eigenvalues) is set to
 * 0 on the rows of the block's Dirichlet mask (monolithic: of both fields' masks) and B's result is 0 there - because that is the
 * operator the Krylov loops see: their residuals are 0 on constrained rows.  pph_extreme_eigenvalues, in contrast, counts the
 * unit rows (an eigenvalue 1 per constrained row).  No free row: PPH_ERR_INVALID ("no free rows").
 * tol <= 0: 1e-4; max_it <= 0: 2000; check_every <= 0: 16 - not the defaults of pph_extreme_eigenvalues: under multigrid the
 * eigenvalues of B A pile up at the upper end, where the Ritz residual shrinks far more slowly than the Ritz value moves
 * ("Preconditioned extremes").  Stopping and breakdown rules: those of pph_extreme_eigenvalues.
 * Positive definiteness: r.Br below -1e-13 max(|alpha_i|, beta_0)^2 at a step, or a negative u.Bu of the start vector, means
 * that B is not positive definite on the Krylov space: PPH_ERR_INVALID with a message, not a breakdown.
 * out[0] lambda_min, out[1] lambda_max of B A on the free rows, out[2] steps taken, out[3] 1 converged / 0 stopped at max_it
 * (values still returned), out[4] 1 after a breakdown, out[5], out[6] the final estimates |beta_m s_m| of the two ends (0 after
 * a breakdown), out[7] ms on the device (event pair, set-up excluded), out[8] rows of the T the values were taken from,
 * out[9] ms of the preconditioner's set-up (hierarchy or factorisation; 0 when it was up to date).
 * fp64, no floating-point atomics: two calls give the same bits.  Memory: 5 vectors of nrows and 3 max_it doubles (device and
 * pinned) plus what the preconditioner owns; the call's own buffers are released on return. */
int pph_preconditioned_extremes(pph_ctx* ctx, int which, int pc_type, int mg_smooth, double tol, int max_it, int check_every,
                                double* out /* [10], host */);
/* host only, no device touched (like pph_asm_wave_map): smallest and largest eigenvalue of the symmetric
 * tridiagonal (alpha[0..m), beta[0..m-1)) by Sturm bisection and the LAST component of their normalised eigenvectors (inverse
 * iteration); out4 = {theta_min, theta_max, s_min_last, s_max_last} */
int pph_tridiag_extremes(const double* alpha, const double* beta, int m, double* out4);

/* ---- error norms (post-processing) -----------------------------------------------------------------
 * replaces: l2_error() / h1_seminorm_error() (reference src/perphil/utils/postprocessing.py:89-124) for
 * the manufactured pressures of src/perphil/utils/manufactured_solutions.py:39-51 (2D), :87-88 (3D).
 * `nodal_host`: the n nodal values of p1_h (field 0) or p2_h (field 1); nq-point Gauss rule per
 * direction (1..8) on quadrilateral / hexahedral cells, collapsed onto the simplex (Duffy transform) on
 * triangles / tetrahedra. */
int pph_error_norms_mms(pph_ctx* ctx, int field, const double* nodal_host, double k1, double k2, double beta,
                        double mu, int nq, double* l2_out, double* h1s_out);
/* The same two norms against ANY exact field, sampled by the caller at the quadrature points
 * replaces: l2_error / h1_seminorm_error for an arbitrary UFL expression (reference src/perphil/utils/postprocessing.py:89-124:
 * sqrt(assemble((p_h - p)^2 dx)), sqrt(assemble(|grad p_h - grad p|^2 dx))) and l2_errors_against_reference
 * (src/perphil/experiments/iterative_bench.py:340-362).  pph_quadrature_points writes the physical coordinates of the
 * nq^dim points of the cells [cell_begin, cell_begin + cell_count) to xq_host[((cell - cell_begin) npts + q) dim + d]
 * (same rule and point order as pph_error_norms_mms); the caller evaluates its field (and gradient) there and
 * pph_error_norms_sampled returns the SQUARED partial norms over those cells: exact_q_host[(cell - cell_begin) npts + q],
 * grad_q_host[((cell - cell_begin) npts + q) dim + d]; either may be NULL (zero field / zero gradient), so the norms of
 * a finite-element function itself come from the same call.  Chunking the cell range bounds the host arrays; nodal_host may
 * be NULL from the second chunk on: the nodal field uploaded by the previous call on this context is used again. */
int pph_quadrature_points(pph_ctx* ctx, int nq, int64_t cell_begin, int64_t cell_count, double* xq_host);
int pph_error_norms_sampled(pph_ctx* ctx, const double* nodal_host, int nq, int64_t cell_begin, int64_t cell_count,
                            const double* exact_q_host, const double* grad_q_host, double* l2sq_out, double* h1sq_out);
/* The same norms of a nodal field held in DEVICE memory (caller-owned, n local values; read on the context stream, not
 * uploaded).  On a slab context (multi-GPU) they are collective: every rank calls, the ghost planes of a copy of the field
 * are refreshed from their owners, each rank integrates over the cells it owns (the cell layer below its lowest owned node
 * plane belongs to the neighbour) and the squared partials are summed over the ranks through the communication hooks.
 * pph_error_norms_sampled_device walks the owned cells in chunks, as pph_error_norms_sampled does: a call with nodal_dev
 * starts a sequence (the field must stay valid until its last call; on a slab its ghost planes are refreshed here, once:
 * collective), a call with NULL continues it; every call adds the squared partials of its cells (inside the owned cells;
 * cell_count 0 allowed) to the sequence's sums and returns them - this rank's own, or, on the call with last != 0, summed
 * over the ranks (collective) and the sequence ends.  Ranks may make different numbers of calls in between.  The samples
 * stay host arrays. */
int pph_error_norms_mms_device(pph_ctx* ctx, int field, const double* nodal_dev, double k1, double k2, double beta,
                               double mu, int nq, double* l2_out, double* h1s_out);
int pph_error_norms_sampled_device(pph_ctx* ctx, const double* nodal_dev, int nq, int64_t cell_begin, int64_t cell_count,
                                   const double* exact_q_host, const double* grad_q_host, int last, double* l2sq_out,
                                   double* h1sq_out);

/* Darcy velocity u = -conductivity * grad(p_h), L2-projected onto the CG-1 vector space of the mesh
 * replaces: calculate_darcy_velocity_from_pressure() (reference src/perphil/utils/postprocessing.py:34-63,
 * fd.project(-k grad p, VectorFunctionSpace(mesh, "CG", 1))).  p_host: n nodal pressures; u_host: [n][dim]
 * (node-major, like a Firedrake vector Function's dat).  Mass-matrix solves run to rtol 1e-13. */
int pph_darcy_velocity(pph_ctx* ctx, const double* p_host, double conductivity, double* u_host);
/* the same projection from a DEVICE pressure p_dev (n values) into a DEVICE u_dev ([n][dim], node-major); both caller-owned,
 * the last writes to u_dev are enqueued on the context stream */
int pph_darcy_velocity_device(pph_ctx* ctx, const double* p_dev, double conductivity, double* u_dev);

/* Point evaluation: values and, when grad is not NULL, gradients of a finite-element function at m arbitrary points
 * replaces: Function.at of Firedrake, which slice_along_x samples (reference src/perphil/utils/postprocessing.py:66-86).
 * Works on whichever mesh the context holds (CG-1 or degree 2; single context).  nodal: [n][ncomp] (node-major: the CG-1
 * vector space's layout; a scalar field is ncomp = 1); x: [m][dim]; val: [m][ncomp]; grad: NULL or [m][ncomp][dim].
 * Location, per direction e: t_e = x_e n_e, box c_e = clamp(floor(t_e), 0, n_e - 1), box-local xi_e = t_e - c_e.  A point
 * with some xi_e outside [-tol, 1 + tol] (tol >= 0, box-local units; 1e-12 is the Python default) is OUTSIDE: all its outputs
 * are NaN, and *n_outside receives the number of such points.  Inside points are clamped to [0, 1].  Sub-cells: triangle 0
 * {0,1,2} where xi_x + xi_y <= 1, else 1 {1,3,2}; the Kuhn tetrahedron whose path 0 -> 7 follows the descending order of
 * (xi_x, xi_y, xi_z).  Ties: a point on a face shared by sub-cells of a box belongs to the LOWEST sub-cell index, a point on
 * a face between two boxes to the upper box; values are continuous there, so this shows in gradients only.
 * The host variant copies everything in and out; the device variant reads and writes caller-owned device arrays on the
 * context stream and returns after the stream has finished with them (the count is read back). */
int pph_eval_points(pph_ctx* ctx, const double* nodal_host, int ncomp, const double* x_host, int64_t m, double tol,
                    double* val_host, double* grad_host, int64_t* n_outside);
int pph_eval_points_device(pph_ctx* ctx, const double* nodal_dev, int ncomp, const double* x_dev, int64_t m, double tol,
                           double* val_dev, double* grad_dev, int64_t* n_outside);

/* Pathlines and travel times (perphil_amd/csrc/pph_trace.hip; no reference counterpart: the reference draws fd.quiver of the
 * projected velocity, src/perphil/utils/postprocessing.py:34-63): m particles carried by v(x) = scale * u_h(x), u_h the CG-1
 * vector field u [n][dim] (node-major, what pph_darcy_velocity writes) of the context's degree-1 mesh, from the seeds x0
 * [m][dim].  A mesh is enough (no Dirichlet data, no assembled system); single context.  Classical RK4, fixed step dt > 0,
 * fp64, points located by pph_eval_points' rule.  INSIDE: every coordinate in [0, 1] (NaN is outside; no tolerance).
 * A step from x: k1 = v(x); |k1|_2 <= min_speed ends the particle (status 2).  x2 = x + dt/2 k1, x3 = x + dt/2 k2,
 * x4 = x + dt k3, xn = x + dt/6 (k1 + 2 k2 + 2 k3 + k4); all four inside: x = xn, time += dt, length += |xn - x|_2.  Otherwise the
 * exit step from x along k1: theta = min_e d_e / |k1_e| over k1_e != 0, d_e the distance to the face k1_e points at (lowest
 * direction on a tie); theta <= dt: x += theta k1, that coordinate set to exactly 0 or 1, time += theta, length += theta |k1|,
 * status 1 with the side numbered as pph_boundary_flux numbers sides; theta > dt: the Euler step x = clamp(x + dt k1, 0, 1),
 * time += dt, length += the distance moved, and the particle goes on.  Every step counts in steps; a particle at max_steps
 * ends with status 0.  A seed that is not inside: status 3, 0 steps, NaN end / time / length.
 * status[p] = status | side << 8 (side 0 unless exited).  counts [4] (host): particles per status.  record_every = r > 0 and
 * path not NULL: path[j][p][:] = position after j r steps, j = 0 .. max_steps / r; slots a particle never reaches hold NaN.
 * One launch advances the live particles by at most `chunk` steps and compacts the survivors; no output depends on chunk
 * or on the run: two calls give the same bits.  m <= 2^31 - 1; m == 0 is valid.  PPH_ERR_INVALID with a message: no mesh,
 * world != 1, a degree-2 context, dt not finite or <= 0, scale zero or not finite, max_steps < 1, chunk < 1, record_every < 0,
 * min_speed < 0 or NaN, NULL buffers with m > 0.  The host variant uploads, runs the device variant and copies back; the
 * device variant works on caller-owned device arrays on the context stream and returns after the stream has finished. */
int pph_trace_pathlines(pph_ctx* ctx, const double* u_host, double scale, const double* x0_host, int64_t m, double dt,
                        int32_t max_steps, double min_speed, int32_t chunk, int32_t record_every, double* end_host,
                        double* time_host, double* length_host, int32_t* steps_host, int32_t* status_host, double* path_host,
                        int64_t* counts);
int pph_trace_pathlines_device(pph_ctx* ctx, const double* u_dev, double scale, const double* x0_dev, int64_t m, double dt,
                               int32_t max_steps, double min_speed, int32_t chunk, int32_t record_every, double* end_dev,
                               double* time_dev, double* length_dev, int32_t* steps_dev, int32_t* status_dev, double* path_dev,
                               int64_t* counts);

/* ---- mass balance (post-processing; perphil_amd/csrc/pph_flux.hip) --------------------------------------------
 * No reference counterpart: the reference stops at pressures and a projected velocity.  These stand beside
 * calculate_darcy_velocity_from_pressure() (reference src/perphil/utils/postprocessing.py:34-63: the same flux
 * -conductivity grad p_h, integrated here instead of projected) and the model's mass transfer xi = beta/mu (p1 - p2)
 * (reference src/perphil/forms/dpp.py:27).  They work on whichever mesh the context holds (CG-1 or degree 2, all four cell
 * kinds), need neither Dirichlet data nor an assembled system, and require a single context (a mesh, world == 1:
 * PPH_ERR_INVALID with a message otherwise).  fp64, no floating-point atomics: two calls give the same bits.  The host
 * variants upload their field and run the device variant; the device variants read caller-owned device arrays on the context
 * stream and return after the stream has finished with them. */
/* out[0] = int p_h dx over the unit square / cube (postprocessing.py:34-63 integrates nothing; dpp.py:27 is the integrand of the
 * transfer T = beta/mu (int p1 - int p2)); nodal: n values; exact for the finite-element function */
int pph_integrate(pph_ctx* ctx, const double* nodal_host, double* out /* [1], host */);
int pph_integrate_device(pph_ctx* ctx, const double* nodal_dev, double* out /* [1], host */);
/* out[s - 1] = F_s = int_{side s} -conductivity grad p_h . n ds (the integrand of postprocessing.py:34-63 on the boundary), sides
 * numbered as Firedrake numbers UnitSquareMesh / UnitCubeMesh: 1: x = 0, 2: x = 1, 3: y = 0, 4: y = 1, 5: z = 0, 6: z = 1; n the
 * outward axis direction, the gradient that of the cell that owns the facet (a cell on an edge or corner of the domain counts for
 * every side it touches); exact for the finite-element function.  Entries past 2 dim are set to 0.  The work is proportional to
 * the boundary cell layers, not to the mesh. */
int pph_boundary_flux(pph_ctx* ctx, const double* nodal_host, double conductivity, double* out /* [6], host */);
int pph_boundary_flux_device(pph_ctx* ctx, const double* nodal_dev, double conductivity, double* out /* [6], host */);
/* Consistent nodal fluxes: the residual of the UN-ELIMINATED operator of dpp.py:27,57,89 on any mixed field p = (p1, p2),
 *   r1 = (k1/mu) K p1 + (beta/mu) M (p1 - p2),   r2 = (k2/mu) K p2 - (beta/mu) M (p1 - p2),
 * K and M the stiffness and mass matrices without Dirichlet rows (pph_get_csr which = 1, 2; integrated on demand and kept by
 * the mesh, like pph_darcy_velocity's of postprocessing.py:34-63).  p, r: 2n values, field-major like the solution.  r_f[i] is
 * minus the outward flux of network f weighted with phi_i: 1^T r1 = T = -1^T r2 with T = beta/mu (int p1 - int p2) for any
 * field, and at a converged solution the entries on free nodes are the solver's residual. */
int pph_dpp_nodal_flux(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p_host, double* r_host);
int pph_dpp_nodal_flux_device(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p_dev, double* r_dev);

/* ---- adjoint solves and parameter gradients (perphil_amd/csrc/pph_adjoint.hip) ----------------------------------
 * No reference counterpart: the reference solves for given k1, k2, beta, mu (src/perphil/solvers/solver.py:30-76) and cannot say
 * how an output changes with them.  The operator of dpp_form (src/perphil/forms/dpp.py:95-132) is symmetric, so the adjoint of a
 * functional J(p) with g = dJ/dp solves the same assembled system for another right-hand side, F A F lambda = F g (F zeroes the
 * constrained dofs), and with the un-eliminated K and M
 *   dJ/dk1 = -o0 / mu, dJ/dk2 = -o1 / mu, dJ/dbeta = -o2 / mu, dJ/dmu = (k1 o0 + k2 o1 + beta o2) / mu^2 (= lambda^T A p: 0 at a
 *   converged solution), dJ/d(boundary value at constrained dof d) = g_d - (A_unel lambda)_d (pph_dpp_nodal_flux of lambda),
 *   o0 = lambda1^T K p1, o1 = lambda2^T K p2, o2 = (lambda1 - lambda2)^T M (p1 - p2).
 *
 * pph_solve_rhs*: x = solution of F A F x = F b for the system of the last pph_assemble_dpp; b, x: 2n values, field-major.  The
 * entries of b on constrained dofs are ignored (masked with the context's Dirichlet masks on the device), x is exactly 0 there.
 * cfg, its checks, the solver paths, info and hist are those of pph_solve_device, whose loops run unchanged: the call exchanges
 * the CONTENTS of the context's right-hand side, lifting (zero) and solution with saved copies, runs that solve and puts the
 * contents back - buffer addresses do not change (captured graphs hold them), and on return the context's right-hand side, lifting
 * and current solution hold the bits they held before: a pph_solve_device afterwards returns the bits it would have returned
 * without the call.  A right-hand side that is zero on every free dof gives x = 0, iterations = 0, converged = 1 without entering
 * a Krylov loop.  PPH_ERR_INVALID with a message: no assembled system, world != 1, a NULL buffer, b == x.  Memory: three vectors
 * of 2n, released on return. */
int pph_solve_rhs_device(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* b_dev /* 2n */, double* x_dev /* 2n */,
                         pph_solve_info* info, double* hist, int hist_cap);
int pph_solve_rhs(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* b_host, double* x_host, pph_solve_info* info,
                  double* hist, int hist_cap);
/* out = {o0, o1, o2} above, as integrals of the finite-element functions: int grad lambda1 . grad p1, int grad lambda2 . grad p2,
 * int (lambda1 - lambda2)(p1 - p2); lam, p: 2n values, field-major.  One matrix-free pass over the cells (closed-form element
 * forms of the uniform boxes): four nodal fields and the dof map are read once, nothing of K or M is built or stored.  Works on
 * whichever mesh the context holds (CG-1 or degree 2, all four cell kinds), needs neither Dirichlet data nor an assembled system.
 * fp64, no floating-point atomics: two calls give the same bits, and so do the host and the device variant.  PPH_ERR_INVALID with
 * a message: no mesh, world != 1, a NULL buffer. */
int pph_dpp_bilinear_device(pph_ctx* ctx, const double* lam_dev /* 2n */, const double* p_dev /* 2n */, double* out /* [3], host */);
int pph_dpp_bilinear(pph_ctx* ctx, const double* lam_host, const double* p_host, double* out /* [3], host */);

/* ---- transient DPP: the right-hand side of a theta step (perphil_amd/csrc/pph_transient.hip) ---------------------
 * No reference counterpart: the reference solves the steady state of dpp_form (src/perphil/forms/dpp.py:95-132).  With a storage
 * coefficient S_f > 0 per network,
 *   S1 dp1/dt - div(k1/mu grad p1) + beta/mu (p1 - p2) = 0,   S2 dp2/dt - div(k2/mu grad p2) - beta/mu (p1 - p2) = 0,
 * the theta scheme (1/2 <= theta <= 1) in delta form solves (Sigma M / dt + theta A) d = -F A_unel p^n, p^{n+1} = p^n + d, where
 * A_unel is the operator of pph_dpp_nodal_flux and F zeroes the dofs the context's Dirichlet sets constrain.  These calls form
 *   b = -F A_unel p:   b1 = -F1 ((k1/mu) K p1 + (beta/mu) M (p1 - p2)),   b2 = -F2 ((k2/mu) K p2 - (beta/mu) M (p1 - p2))
 * for both fields in one pass; p, b: 2n values, field-major; the entries of b on constrained dofs are exactly 0.  A mesh is enough
 * (no assembled system); without Dirichlet data F is the identity.  Degree-1 meshes: matrix-free - one work item per node gathers
 * from its incident cells with the closed-form element matrices of the canonical cell, cells outside the box skipped by index
 * arithmetic; neither K nor M is stored and the dof map is not read.  Degree 2, or option "asm_uniform" 0: the CSR walk of
 * pph_dpp_nodal_flux on the stored K and M, then mask and sign.  fp64, no floating-point atomics: two calls give the same bits.
 * PPH_ERR_INVALID with a message: no mesh, world != 1, a NULL buffer, p == b, mu == 0.  The host variant copies in and out; the
 * device variant works on caller-owned device arrays on the context stream and returns after the stream has finished with them. */
int pph_dpp_step_rhs_device(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p_dev /* 2n */,
                            double* b_dev /* 2n */);
int pph_dpp_step_rhs(pph_ctx* ctx, double k1, double k2, double beta, double mu, const double* p_host, double* b_host);
/* The step loop.  pph_transient_begin checks S_f > 0, dt > 0, 1/2 <= theta <= 1 (backward Euler 1, Crank-Nicolson 1/2), assembles
 * the step operator Sigma M / dt + theta A through pph_assemble_dpp_shifted(theta k1, theta k2, theta beta, mu, S1 / dt, S2 / dt,
 * monolithic) and records the steady coefficients.  pph_transient_steps* advances p (2n values, field-major, in / out) by up to
 * nsteps steps: the constrained entries of p are first overwritten with the context's Dirichlet values; the CONTENTS of the
 * context's right-hand side, lifting and solution are exchanged with saved copies ONCE per call, as pph_solve_rhs does per solve
 * (addresses unchanged; on return they hold the bits they held before); per step the kernel above writes b_s = -F A_unel p^s
 * straight into the context's right-hand side, the solve loop of pph_solve_device runs on the path cfg names (same checks), and
 * one kernel does p += d and leaves the partial sums of ||d||^2.  norms[s] = {||b_s||_2, ||d_s||_2}; infos[s]: the solve of
 * step s (either may be NULL).  A step whose right-hand side is zero on every free dof takes no solve (d = 0, iterations 0,
 * converged 1).  The loop stops before step s when ||b_s|| <= steady_tol ||b_0|| (steady_tol <= 0: never; b_0: the first right-hand side
 * formed after pph_transient_begin, so that a run split over several calls stops where one call would); *steps_done = steps
 * taken.  No allocation per step; per step the host reads ||b_s||^2 (with it ||d_{s-1}||^2) once, beside the solve's own
 * synchronisations.  A diverged solve ends the loop with PPH_ERR_DIVERGED: p holds the last completed step, *steps_done is set.
 * PPH_ERR_INVALID with a message: steps before begin; an assembly or a change of the Dirichlet sets in between; world != 1; a NULL
 * buffer (p, cfg, steps_done); nsteps < 1; bad S, dt, theta.  Memory: three vectors of 2n, released on return.  The host variant
 * copies p in and out. */
int pph_transient_begin(pph_ctx* ctx, double k1, double k2, double beta, double mu, double S1, double S2, double theta, double dt,
                        int monolithic);
int pph_transient_steps_device(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_dev /* 2n, in/out */, int nsteps,
                               double steady_tol, pph_solve_info* infos /* [nsteps] or NULL */,
                               double* norms /* [nsteps][2] or NULL */, int* steps_done);
int pph_transient_steps(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_host /* 2n, in/out */, int nsteps, double steady_tol,
                        pph_solve_info* infos, double* norms, int* steps_done);

/* pph_transient_steps with one more argument: traj, [nsteps + 1][2n].  Row 0 receives p after the Dirichlet values were written,
 * row s + 1 the state after step s; rows past *steps_done + 1 are not written.  The device variant takes a caller-owned device
 * array; p, norms, infos and the context are left bit for bit as pph_transient_steps leaves them. */
int pph_transient_steps_record_device(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_dev /* 2n, in/out */, int nsteps,
                                      double steady_tol, pph_solve_info* infos, double* norms, int* steps_done,
                                      double* traj_dev /* [nsteps + 1][2n] */);
int pph_transient_steps_record(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_host /* 2n, in/out */, int nsteps,
                               double steady_tol, pph_solve_info* infos, double* norms, int* steps_done, double* traj_host);

/* ---- transient adjoint (perphil_amd/csrc/pph_transient_adjoint.hip) ---------------------------------------------
 * Gradients of J = sum_{s=0..N} j_s(p_s) over a trajectory of pph_transient_steps, G_s = dj_s/dp_s.  T = Sigma M / dt + theta A is
 * symmetric: with q_N = F G_N, for s = N-1 down to 0
 *   w_s = T^-1 q_{s+1};  pm = p_s + theta d_s, d_s = p_{s+1} - p_s;
 *   terms[s] = {w1^T K pm1, w2^T K pm2, (w1 - w2)^T M (pm1 - pm2), w1^T M d1, w2^T M d2};
 *   q_s = F G_s + q_{s+1} - F A_unel w_s;  Wsum += w_s,
 * and with O_q = sum_s terms[s][q] (summed by the caller in the order s = N-1 down to 0)
 *   dJ/dk1 = -O0/mu, dJ/dk2 = -O1/mu, dJ/dbeta = -O2/mu, dJ/dmu = (k1 O0 + k2 O1 + beta O2)/mu^2, dJ/dS1 = -O3/dt, dJ/dS2 = -O4/dt,
 *   dJ/dp_0 = q_0 on free dofs, dJ/d(boundary value at constrained dof c) = sum_s (G_s)_c - (A_unel Wsum)_c (pph_dpp_nodal_flux).
 *
 * pph_transient_bilinear*: out5 = the five forms of ONE step for any w, p0 (= p_s), p1 (= p_{s+1}) (2n values each, field-major) in
 * one matrix-free pass over the cells; a mesh is enough.  CG-1 and degree 2, all four cell kinds.  fp64, no atomics, the grid is a
 * function of the mesh alone: two calls give the same bits, and so do the host and the device variant. */
int pph_transient_bilinear_device(pph_ctx* ctx, const double* w_dev, const double* p0_dev, const double* p1_dev, double theta,
                                  double* out5 /* [5], host */);
int pph_transient_bilinear(pph_ctx* ctx, const double* w_host, const double* p0_host, const double* p1_host, double theta,
                           double* out5 /* [5], host */);
/* The transpose of pph_eval_points: out[node * ncomp + k] += sum_m phi_node(x_m) c[m * ncomp + k] (out is ADDED to).  Location rule,
 * tie-breaks and tol are pph_eval_points'; a point outside contributes nothing and is counted in *n_outside.  One workgroup takes
 * the points in index order (lanes: the local basis functions; a barrier between points): no floating-point atomics, bitwise
 * reproducible, any number of points per cell, duplicates included.  The cost is LINEAR in m - the points are taken one after
 * the other - which suits observation wells (tens to thousands of points), not fields of points. */
int pph_eval_points_adjoint_device(pph_ctx* ctx, const double* x_dev /* [m][dim] */, int64_t m, const double* c_dev /* [m][ncomp] */,
                                   int ncomp, double tol, double* out_dev /* [n][ncomp], in/out */, int64_t* n_outside);
int pph_eval_points_adjoint(pph_ctx* ctx, const double* x_host, int64_t m, const double* c_host, int ncomp, double tol,
                            double* out_host, int64_t* n_outside);
/* The backward loop above on the step operator of the last pph_transient_begin (same epoch checks as pph_transient_steps).  traj:
 * [N + 1][2n] as pph_transient_steps_record wrote it.  G_s = g[s] (g: [N + 1][2n], or NULL) + E^T obs_c[s] (obs_x: [m][dim],
 * obs_c: [N + 1][m][2] = weights of (p1, p2) at the points, or NULL; points located with obs_tol as pph_eval_points does); at least
 * one of g and obs_c must be given.  terms: [N][5] on the host, written on the device per step and fetched once at the end (rows
 * of steps not reached are 0); q0: 2n; wsum: 2n or NULL; infos[s]: the solve of step s, or NULL.  *steps_done = backward steps
 * completed.  The CONTENTS of the context's right-hand side, lifting and solution are exchanged once per call and put back bit for
 * bit; the solve loop of pph_solve_device runs on the path cfg names; a q that is zero on every free dof takes no solve (w = 0).  Per
 * step the host reads ||q||^2 once, beside the solve's own synchronisations.  A diverged solve ends the loop with
 * PPH_ERR_DIVERGED (q0 then holds the last completed q).  Memory: seven vectors of 2n, released on return; the host variant also
 * holds the trajectory and g on the device for the call. */
int pph_transient_adjoint_device(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* traj_dev, const double* g_dev,
                                 const double* obs_x_dev, int64_t m, const double* obs_c_dev, double obs_tol, int nsteps,
                                 double* terms /* [nsteps][5], host */, double* q0_dev, double* wsum_dev,
                                 pph_solve_info* infos /* [nsteps] or NULL */, int* steps_done);
int pph_transient_adjoint(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* traj_host, const double* g_host,
                          const double* obs_x_host, int64_t m, const double* obs_c_host, double obs_tol, int nsteps, double* terms,
                          double* q0_host, double* wsum_host, pph_solve_info* infos, int* steps_done);

/* ---- sources of the transient runs: wells and distributed sources (perphil_amd/csrc/pph_sources.hip) ------------------
 * no reference counterpart (the reference's dpp_form has no right-hand side beyond the Dirichlet lifting).  With load vectors L_k
 * (2n values, field-major, constant in time) and rates r_k(t) (q > 0 injects) a theta step solves
 *   (Sigma M / dt + theta A) d = F (-A_unel p^s + sum_k c[s][k] L_k),   c[s][k] = theta r_k(t_{s+1}) + (1 - theta) r_k(t_s).
 * F drops what falls on constrained dofs: a well on a Dirichlet node pumps into the boundary condition.
 *
 * pph_sources_set* replaces the context's source set: n_dense load vectors [n_dense][2n] (copied into the context) and m point
 * loads, L[dof] = phi_dof(x_p) on the nodes of the cell that holds x_p in network field[p] (0 or 1) - the transpose of
 * pph_eval_points: its location rule, tie-breaks and tol; CG-1 and degree 2, all four cell kinds.  A point outside the mesh is
 * counted in *n_outside and gets an empty row (it stays a source: its coefficient multiplies nothing).  K = n_dense + m sources:
 * coefficient k < n_dense belongs to dense load k, coefficient n_dense + p to point p.  `field` is a HOST array in both variants;
 * dense and x are host arrays (pph_sources_set) or device arrays (pph_sources_set_device).  The point rows (m x nodes-per-cell
 * entries) are formed by one kernel, fetched once (16 bytes per entry) and regrouped on the host by dof (stable: dof first, then
 * point index) into a CSR that is uploaded (12 bytes per entry, 16 per touched dof): a set-up cost, one sort of those entries.  The set lives on the context, independent of assemblies and of
 * pph_transient_begin; pph_mesh_build* clears it.  A refused call leaves the set as it was.  pph_sources_count: *count = K, or -1
 * when the context holds no set.  PPH_ERR_INVALID with a message: no mesh, world != 1, a NULL buffer with a non-zero count (or
 * n_outside NULL), a negative count, a field index outside {0, 1}, tol outside [0, 0.5), more than 65535 dense loads. */
int pph_sources_set_device(pph_ctx* ctx, const double* dense_dev /* [n_dense][2n] */, int64_t n_dense,
                           const double* x_dev /* [m][dim] */, const int32_t* field /* [m], host */, int64_t m, double tol,
                           int64_t* n_outside);
int pph_sources_set(pph_ctx* ctx, const double* dense_host, int64_t n_dense, const double* x_host, const int32_t* field, int64_t m,
                    double tol, int64_t* n_outside);
int pph_sources_clear(pph_ctx* ctx);
int pph_sources_count(pph_ctx* ctx, int64_t* count);
/* b += F sum_k coef[k] L_k for one coefficient row coef [K] (host); b: 2n values, in place.  What the step loop launches per step.
 * Dense part: one grid-stride pass, every L_k read once, b read and written once (16-byte accesses where b_dev is 16-byte
 * aligned, 8-byte ones otherwise: same arithmetic, same bits), the sum over k in index order.  Point part: one work item per touched dof walks its CSR row in order.  Either part is skipped when empty.  fp64, no
 * floating-point atomics: two calls give the same bits, the result does not depend on the grid, host and device variant agree
 * bit for bit.  PPH_ERR_INVALID with a message: no mesh, world != 1, no source set, a NULL buffer. */
int pph_sources_apply_device(pph_ctx* ctx, const double* coef /* [K], host */, double* b_dev /* 2n, in/out */);
int pph_sources_apply(pph_ctx* ctx, const double* coef, double* b_host);
/* pph_transient_steps_record* with the context's source set: coef [nsteps][K] (host) is uploaded once per call (it shares the
 * call's one allocation: none and no host-to-device copy per step), and b_s += F sum_k coef[s][k] L_k between the kernel that
 * forms -F A_unel p^s and the norm of b_s: norms[s][0] is the norm of the full right-hand side, which is also what the zero
 * right-hand-side shortcut and steady_tol look at.  traj may be NULL (no recording).  Everything else is the contract of
 * pph_transient_steps.  Also PPH_ERR_INVALID with a message: no source set, or one of another size than K; coef NULL with K > 0. */
int pph_transient_steps_sources_device(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_dev /* 2n, in/out */, int nsteps,
                                       double steady_tol, pph_solve_info* infos, double* norms, int* steps_done,
                                       double* traj_dev /* [nsteps + 1][2n] or NULL */, const double* coef /* [nsteps][K], host */,
                                       int64_t K);
int pph_transient_steps_sources(pph_ctx* ctx, const pph_solver_cfg* cfg, double* p_host /* 2n, in/out */, int nsteps,
                                double steady_tol, pph_solve_info* infos, double* norms, int* steps_done, double* traj_host,
                                const double* coef, int64_t K);
/* pph_transient_adjoint* with the rate gradients: src_grad [nsteps][K] (host), src_grad[s][k] = w_s^T F L_k, written on the device
 * per backward step and fetched once at the end, as terms are (rows of steps not reached are 0).  Dense loads: a masked dot
 * product with per-workgroup partial sums in a fixed order; points: one work item per point over the point rows kept from the
 * set-up, constrained dofs skipped.  A source enters neither the recursion nor the parameter gradients (it depends neither on
 * the state nor on the parameters): everything else is the contract of pph_transient_adjoint.  dJ/dr_k(t_j) = theta
 * src_grad[j-1][k] + (1 - theta) src_grad[j][k], rows outside 0 .. nsteps-1 taken as 0.  Also PPH_ERR_INVALID with a message:
 * no source set, or one of another size than K; src_grad NULL with K > 0. */
int pph_transient_adjoint_sources_device(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* traj_dev, const double* g_dev,
                                         const double* obs_x_dev, int64_t m, const double* obs_c_dev, double obs_tol, int nsteps,
                                         double* terms, double* q0_dev, double* wsum_dev, pph_solve_info* infos, int* steps_done,
                                         double* src_grad /* [nsteps][K], host */, int64_t K);
int pph_transient_adjoint_sources(pph_ctx* ctx, const pph_solver_cfg* cfg, const double* traj_host, const double* g_host,
                                  const double* obs_x_host, int64_t m, const double* obs_c_host, double obs_tol, int nsteps,
                                  double* terms, double* q0_host, double* wsum_host, pph_solve_info* infos, int* steps_done,
                                  double* src_grad, int64_t K);

/* ---- multi-GPU communication hooks -------------------------------------------------------------
 * replaces: PETSc's implicit VecScatter halo exchange and VecDot all-reduce under mpiexec (never run in
 * the reference).  One context per rank holds one cell slab (pph_mesh_build with
 * z_cell_begin/z_cell_count/ghost_lo/ghost_hi).  The library calls
 *   halo(user, vec, plane_elems, send_lo, recv_lo, send_hi, recv_hi): offsets (in elements, -1 = no
 *        neighbour) into the DEVICE vector `vec`: send [send_lo, +plane) to rank-1 and receive its
 *        top owned plane into [recv_lo, +plane); likewise send_hi/recv_hi with rank+1.  The context
 *        stream is idle when the callback runs; the callback returns when the data have arrived.
 *   allreduce(user, vals, count): sum `count` HOST doubles over all ranks, in place.
 * Both return 0 on success.  perphil_amd/distributed.py implements them over torch.distributed. */
typedef int (*pph_halo_fn)(void* user, double* vec, int64_t plane_elems, int64_t send_lo, int64_t recv_lo,
                           int64_t send_hi, int64_t recv_hi);
typedef int (*pph_allreduce_fn)(void* user, double* vals, int64_t count);
int pph_comm_set_callbacks(pph_ctx* ctx, int rank, int world, pph_halo_fn halo, pph_allreduce_fn allreduce,
                           void* user);
/* RCCL transport (default on the multi-GPU node): the library issues grouped ncclSend/ncclRecv of the
 * neighbour planes and ncclAllReduce of the reduction scalars on its own stream.  librccl is resolved with
 * dlopen (`libpath` may be NULL/empty: default search, then /opt/rocm/lib).  Rank 0 draws the 128-byte
 * unique id, the launcher broadcasts it, every rank calls pph_comm_init_rccl; pph_comm_selftest verifies
 * a send/recv to self and an all-reduce on the context stream. */
int pph_rccl_available(const char* libpath);   /* 0 when librccl loads with every entry point used here: every rank
                                                * checks (and the launcher agrees on the result) BEFORE any rank enters
                                                * ncclCommInitRank */
int pph_rccl_unique_id(const char* libpath, uint8_t* id128);
int pph_comm_init_rccl(pph_ctx* ctx, int rank, int world, const uint8_t* id128, const char* libpath);
/* straight-line self-test: every rank issues all three phases (to self, both slab neighbours, all-reduce) whatever
 * fails on the way, and reports afterwards; ranks_seen (optional) = world size observed by the all-reduce */
int pph_comm_selftest(pph_ctx* ctx);
int pph_comm_selftest2(pph_ctx* ctx, int* ranks_seen);
/* halo exchanges and all-reduces of the last solve, and the sticky communication status: after the first failed
 * exchange / reduction on a context every solve returns PPH_ERR_COMM until the transport is set up again */
int pph_comm_stats(pph_ctx* ctx, int64_t* halo_exchanges, int64_t* allreduces, int* status);
/* with option "time_comm" on: summed durations (ms) of the last solve's halo exchanges (out4[0]) and all-reduces (out4[1])
 * and how many of each were timed (out4[2], out4[3]).  RCCL transport: device time between two HIP events on the issuing
 * stream (an exchange overlapped with interior rows counts its full duration on the communication stream); callback
 * transport: host time inside the callback.  Lets a measured scaling curve be split into communication and the rest. */
int pph_comm_times(pph_ctx* ctx, double* out4);

/* ---- stats ---------------------------------------------------------------------------------
 * replaces: PETSc -log_view event times scraped by reference src/perphil/experiments/petsc_profiling.py:302-447.
 * out[0] mesh+pattern ms, [1] integration ms (fused assembly: the whole assembly), [2] elimination/blocks ms of
 * the two-step path (0 when fused), [3] last solve ms;
 * SpMV accounting of the last solve per kernel variant v (0: plain, 1: fused with the p.Ap dot):
 * out[4+3v] sum of per-launch durations in ms (0 unless option "time_spmv" is on), out[5+3v] launches,
 * out[6+3v] algorithmic bytes (CSR launches: 12 nnz + 20 nrows; stencil-ELL launches: (8 S + 16 + e) nrows with S the
 * STORED slots per row - 14 of 27 for hexahedra in symmetric storage - and e = 8 / 16 / 32..48 for the residual,
 * Jacobi-update and Picard-bookkeeping epilogues' extra vectors); out[10] halo exchanges of the last solve;
 * out[11..13] the same three figures (ms, launches, bytes; both variants together) for the launches on
 * fine-level operators only (rows >= nodes of the mesh), i.e. without the coarser multigrid levels;
 * out[14] products of the last solve launched as interior + boundary rows (option "halo_overlap", slabs only);
 * out[15] 1 when the stencil-ELL blocks of the last assembly use symmetric storage;
 * out[16] the most partial sums a split product has written into one reduction slot so far (<= option "part_cap");
 * out[17] stencil-ELL operators (fine blocks + multigrid levels) whose products run on a row dictionary (option
 * "sell_dict": distinct rows stored once + a 2-byte class per row; their launches count (2 + 16 + e) nrows bytes),
 * out[18] distinct rows of A11 found by the last build (0: not tried), out[19] its status on the device (1 in use,
 * 0 not built, -1 more distinct rows than the cap, -2 a row failed the bitwise check: plain storage is used);
 * out[20] ms spent so far in FIRST builds of row dictionaries (hash build + table + first bitwise check + the read-back of
 * the verdict; once per operator, mesh and Dirichlet-set pair - a symbolic-phase cost like the pattern of a CSR matrix),
 * out[21] how many such builds; out[22] 1 when the products of A11 take the classes of the interior planes from the plane below
 * (option "sell_dict_zconst": the class words of four planes only are read - launches count (16 + e) nrows bytes + those);
 * out[23] / out[24] rows the two launches of the fine level's node assembly stored last (straight-line windows / general form;
 * 0: one launch), out[25] rows of that level;
 * out[26] on-chip LU-equivalent block solves of the last solve (cfg.inner_exact on a single context, blocks of at most 4096 rows
 * in stencil-ELL storage: one workgroup runs the whole Jacobi-CG of a block solve, the host does not wait for it), out[27] how
 * many of them ended WITHOUT meeting their tolerance (iteration limit, option "onchip_max_it", or p.Ap <= 0; a zero right-hand
 * side counts as converged) - any such solve sets pph_solve_info.inner_failed = 1 and converged = 0: it is reported, not
 * repeated on the host-driven loop - out[28] their CG iterations summed.  All three are 0 when the path did not run;
 * out[29] CG updates of the last solve launched without the next multigrid cycle's pre-smoothed first guess (option
 * "presmooth_lazy"), out[30] cycles that ran after such an update and formed the guess themselves, out[31] updates that
 * wrote a guess no cycle read (unpreconditioned-norm CG block solves around the fused cycle; 0 elsewhere);
 * out[32] 1 when the last assembly did not store the operator entries of the fine level's straight-line rows (option
 * "asm_store_values" 0), out[33] launches that wrote such rows because a reader asked, since the context was created,
 * out[34] levels whose row dictionary was refused on the device while their rows were left out - written by the repair launch
 * behind that assembly's last check kernel, counted when the solve's end retires the dictionary;
 * out[35] product launches of the last solve (or pph_pc_apply) whose smoothing epilogue took its factors 1 / a_ii from a row
 * dictionary's table of inverse diagonals instead of the dinv array (option "sell_dict_dinv"; launches recorded into a
 * captured graph count once, when recorded);
 * out[36] fine-level launches of the last solve (or pph_pc_apply) that swept their vectors descending (option "l3_order";
 * counted like out[35]). */
int pph_get_timers(pph_ctx* ctx, double* out, int n);
/* tuning / profiling switches (no reference counterpart; defaults in brackets):
 *   "op_format" [1]      operator format of the scalar blocks inside block solves / Picard sweeps: 1 stencil-ELL
 *                        (values only, val[slot][row]; written directly by the fused assembly), 0 CSR.  pph_get_csr /
 *                        pph_spmv export CSR either way (converted on demand).
 *   "sell_rpt" [2], "sell_blocks" [4096; z-walk: one per CU], "sell_group" [1]   stencil-ELL SpMV: rows per thread, grid cap, XCD chunk group
 *   "sell_sym" [1]       symmetric blocks store the diagonal and the upper stencil slots only; "sell_sym_slabs" [1]: also
 *                        on slabs, where ghost rows then keep their entries towards owned columns (the mirrors of the
 *                        owned rows' lower entries; operators converted from CSR values stay in full storage there)
 *   "sell_zwalk" [4], "sell_zwalk_min_chunks" [5500], "sell_xmap" [1]   symmetric product on large 3D levels: a workgroup
 *                        walks this many node planes at one in-plane position (>= 1000: a balanced share of a whole z
 *                        column); the in-plane positions of one XCD's workgroups are consecutive
 *   "spmv_lanes" [0 = automatic, 4..64 lanes per CSR row], "spmv_blocks" [0 = 1024 workgroups], "spmv_bench_mode" [0]
 *   "time_spmv" [0]      1: bracket every SpMV launch of a solve with a HIP event pair on the context stream
 *   "asm_kernel" [2]     multilinear assembly: 0 cell-centred scatter-add (atomics), 1 node-centred gather, 2 fused kernels
 *   "asm_tile" [1]       fused multilinear assembly: 1 single-pass tile kernel on levels of at least
 *                        "asm_tile_min_nodes" [30000] nodes (2: on every level), 0 two-pass (element rows + gather)
 *   "asm_affine" [1]     tile kernel: a cell whose parallel edges are equal vectors gets its constant geometry factor once
 *                        per cell; 0: Jacobian at every Gauss point of every cell (the general pass)
 *   "asm_fused" [1]      the node-centred pass writes the eliminated blocks, lifted right-hand side and smoother
 *                        diagonal directly; 0: K and M first, then separate elimination kernels
 *   "asm_keep_km" [0]    1: the fused pass also stores K and M (otherwise they are integrated on demand)
 *   "asm_store_values" [0] 0: an assembly whose rows are checked against the row dictionaries inside the node kernel
 *                        (every assembly after the first on a large uniform-coefficient box) computes and compares the
 *                        operator entries of its straight-line rows but does not store them: the products run on the
 *                        dictionaries.  The entries are written when somebody needs them - a plain product, pph_get_csr,
 *                        "sell_dict_poison", a change of the Dirichlet sets or of an "asm_*" option - and, when a check refuses a
 *                        dictionary on the device, by a launch enqueued behind the check that is empty otherwise
 *                        (pph_get_timers out[32..34]).  Single context, levels of more than 4096 rows.  1: every assembly
 *                        stores every entry.  Results are bitwise the same either way
 *   "invalidate_KM"      drop the integrated K and M so that the next assemble integrates again
 *   "mg_fused" [1]       V(1,1) on stencil-ELL levels: fused smoother / transfer kernels + on-chip tail; 0 general cycle
 *   "mg_tail_rows" [5000] levels with at most min(this, 1024) rows join the single-workgroup tail of the cycle
 *   "coarse_max_it" [500] iteration limit of the coarsest-level Jacobi-CG (reported through inner_failed)
 *   "onchip_max_it" [0]  iteration limit of an on-chip LU-equivalent block solve (rtol 1e-12); 0: 8 n + 64 for n rows.  A solve
 *                        that stops there is reported through inner_failed and pph_get_timers out[27]
 *   "mg_fp32" [0], "mg_replicate_below" [40000 nodes], "coarse_on_device" [1]   multigrid: fp32 copies of the V-cycle
 *                        operators (CSR only), replication threshold of coarse levels on slabs, coarsest solve on the device
 *   "mg_replicate_rows_per_rank" [40000], "mg_replicate_cap" [1e6]   slabs: a level is also replicated when its share per
 *                        rank is at most this many nodes (its kernels are shorter than one halo exchange) and the whole
 *                        level has at most mg_replicate_cap nodes; 0 restores the global threshold alone
 *   "time_comm" [0]      1: every halo exchange / all-reduce of a solve is timed (pph_comm_times)
 *   "fetch_spin" [1]     reduction results reach the host through a mapped mirror the host polls; 0: D2H copy + sync
 *   "merge_allreduce" [1] slabs, CG block solves on stencil-ELL operators: the product also sums r.Ap and Ap.Ap, and
 *                        { p.Ap, r.Ap, Ap.Ap, r.r of the previous update } travel in ONE all-reduce; the host forms the next
 *                        r.r by one step of the recurrence (two scalar all-reduces per iteration instead of three)
 *   "presmooth_lazy" [1] unpreconditioned-norm CG block solves around the fused cycle: a CG update also writes the next
 *                        cycle's first guess dinv .* r * w (two of its eight vector passes).  1: not when the host expects the
 *                        update to be the last of its solve - the block's most recent residual contraction would carry the
 *                        residual below the tolerance; at most two such guesses per solve, none while iteration bodies are
 *                        replayed from graphs; a cycle that runs after all forms the guess itself, bit for bit the same.
 *                        2: the update at which the block's previous solve ended.  0: every update writes it
 *   "use_graphs" [1]     launch sequences replayed from captured hipGraphs: ILU(0) sweeps, the launch-only Picard sweeps of
 *                        inner_norm 2, and CG iteration bodies on systems of up to "graph_cg_max_rows" [0] rows (2: always)
 *   "device_scalars" [0] 1: the device-scalar CG branch also over the callback transport (tests)
 *   "halo_overlap" [1]   slabs: products on levels of at least "halo_overlap_min_rows" [200000] rows are launched as
 *                        interior rows + boundary rows; 1: the exchange of the operand's ghost planes runs on a second
 *                        stream while the interior rows are computed, 2: the same launches, exchange first (the two
 *                        give bit-identical results).  The three launches share one reduction slot's partial-sum area:
 *                        their grids are capped so that together they write at most "part_cap" [4096, the area's size;
 *                        tests lower it] partial sums
 *   "sell_dict" [1]      row dictionaries for the symmetric stencil-ELL operators of at least "sell_dict_min_rows" [1e6]
 *                        rows: after an assembly the distinct rows (all 27 / 15 / 9 / 7 coefficients a product would load for a row,
 *                        bit patterns; all four cell kinds) are stored once and every row gets a 2-byte class; every assembly checks every row
 *                        against its class bit for bit; products then read the class instead of the stored values and are
 *                        bit-identical.  More than "sell_dict_cap" [256] distinct rows (graded meshes, node spacing not
 *                        exact in binary) or a failed check: stored values as before.  "sell_dict_walk" [1]: whole-operator
 *                        products on hexahedra keep the x window in registers (k_spmv_dict_walk), "sell_dict_blocks"
 *                        [1024] their grid, "sell_dict_zconst" [1]: where the class of an in-plane position is the same on all
 *                        interior planes (verified on the class array at the build) a step takes its classes from the step
 *                        below instead of loading them; 0 takes effect at once, 1 at the next assembly.
 *                        "sell_dict_dinv" [1] (0 or 1, anything else is refused): the Jacobi-type epilogues of dictionary
 *                        products (the cycle's smoothing products; the Picard sweeps' coupling products that write the next
 *                        solve's first guess) take 1 / a_ii from a table with one entry per class - the class's diagonal entry
 *                        through the assembly's expression, so the same double - instead of streaming the n-entry array;
 *                        coupling products read the class of the DIAGONAL block's dictionary for that.  A dictionary refused
 *                        on the device, no dictionary, slabs: the array as before.  Takes effect at the next launch
 *   "l3_order" [1]       (0 or 1, anything else is refused) single context: a fine-level kernel starts its sweep where the
 *                        kernel before it stopped, so that the vectors both touch are met in the Infinity Cache: the order-free
 *                        elementwise and transfer kernels run their grid-stride loops descending every other launch, the walk
 *                        products (k_spmv_dict_walk) take their ranges in reverse.  Kernels with running sums (the CG update, the
 *                        dot products) stay ascending, the product in front of the update always runs descending, and a cycle's
 *                        restriction and interpolation share a direction.  Only vectors of at least "l3_order_min_rows"
 *                        [4 000 000] rows; no item, range or partial-sum slot changes, so results are bit-identical.
 *                        "l3_walk_order" [1]: 1 the walk's ranges plane-band major (sorted by first plane, then in-plane
 *                        chunk), 0 in their own order.  0: every launch as without the option.  Takes effect at the next launch
 *   "fold_finals" [1]    single context: the final reductions of p.Ap and of the multigrid cycle's r.z are summed inside the
 *                        kernels that consume them instead of by launches of their own (same sums, same order)
 *   "pmg_fused" [1]      PPH_PC_PMG at degree 2: the smoother steps and residuals of the degree-2 level run in the tile kernels
 *                        of pph_pmg.hip (product + Chebyshev recurrence, or product + masked residual, in one pass; lanes
 *                        dealt over the entries of a tile of rows instead of a fixed count per row); 0: the generic
 *                        composition CSR product + vector kernels, for comparison from one build.  "pmg_tile_rows" [32]:
 *                        rows per tile of those kernels on 3D meshes, 32 or 16 (16 measured slower on Q2 64^3)
 *   "transfer_bench"     diagnostic: times `value` launches of the fine-level interpolation / restriction kernels of an existing
 *                        hexahedral hierarchy and prints the result on stderr (tools/r4_transfer_probe.py) */
int pph_set_option(pph_ctx* ctx, const char* name, double value);

#ifdef __cplusplus
}
#endif
#endif /* PERPHIL_HIP_H */
