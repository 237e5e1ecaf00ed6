/*
 * libmldgpu -- MI355X-native (gfx950) batched MLD-MPC solve path.  Plain C ABI: caller-owned,
 * C-contiguous row-major `double` arrays; the library copies in/out and never keeps a host pointer
 * past the call.  Every function returns 0 on success and a negative mld_err on failure; the text of
 * the last error on the calling thread is mld_last_error().  A handle is not thread-safe; distinct
 * handles are.  There is no CPU fallback: without a HIP device every compute entry point fails
 * with MLD_ERR_NO_DEVICE.
 *
 * The reference (michchr/pyhybridcontrol) has no FFI: its seam for this path is the Python call
 * `ConstraintSolvedController.solve()` -> `cvx.Problem.solve()` (controllers/controller_base.py:491-540,
 * :509).  Each entry point below names the reference code it replaces; INTEGRATION.md shows the
 * ctypes binding a maintainer would add on the reference side.
 */
#ifndef MLDGPU_H
#define MLDGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mld_model mld_model_t;
typedef struct mld_problem mld_problem_t;

typedef enum {
    MLD_OK = 0,
    MLD_ERR_INVALID = -1,     /* bad argument / shape */
    MLD_ERR_NO_DEVICE = -2,   /* no HIP device: the product path has no CPU fallback */
    MLD_ERR_UNSUPPORTED = -3, /* e.g. a problem too large for the LDS staging */
    MLD_ERR_HIP = -4,         /* HIP runtime error (text in mld_last_error) */
    MLD_ERR_COMM = -5         /* RCCL error */
} mld_err;

/* per-instance solve status (status_out of mld_solve_batch) */
typedef enum {
    MLD_STATUS_OPTIMAL = 0,
    MLD_STATUS_INFEASIBLE = 1,
    MLD_STATUS_NODE_LIMIT = 2, /* incumbent (if any) returned, gap = obj - lower_bound */
    MLD_STATUS_NUMERICAL = 3,
    MLD_STATUS_UNBOUNDED = 4   /* a free variable rests on the solver's artificial box: objective -inf, the ray's point in v_out
                                  (counted under n_numerical in mld_stats) */
} mld_status;

/* MLD dimensions, models/mld_model.py:149-168 (MldInfo._mld_dim_map): nv = nu+ndelta+nz+nmu;
 * binaries are the trailing nu_l / nmu_l entries of u / mu, all of delta, none of z (:294-345). */
typedef struct {
    int32_t nx, nu, ndelta, nz, nmu, nomega, ny, nc, nu_l, nmu_l;
} mld_dims;

/* flags */
#define MLD_CONDENSE_DEFAULT 0
/* mld_opts.flags: the dense GEMMs of the path -- K3 constraint right-hand sides ([H_x | H_w] [x0 ; w], controllers/
 * controller_base.py:446-450) and K4 quadratic cost pull-back (Gamma' W Gamma, controllers/components/objective_atoms.py:
 * 321-331) -- run on the matrix cores in fp32 (v_mfma_f32_16x16x4_f32: inputs rounded to fp32, fp32 accumulate; relative
 * error ~1e-6 of the largest term) instead of fp64 (v_mfma_f64_16x16x4_f64).  Arrays at the boundary stay `double`; the
 * branch-and-cut itself always runs in fp64 and verifies every returned point against the original fp64 rows. */
#define MLD_F32 1
/* mld_opts.flags: small problems are solved by the LDS-resident wave-per-instance kernel (k_small_milp) instead of the dense-dictionary kernel.
 * Fixed at mld_problem_create like MLD_F32 and composes with it (K3 may run in fp32, the solver stays fp64).  It takes effect when the
 * problem is ELIGIBLE -- its dense dictionary with the per-basis state and the search stack fits the 16 KB of LDS a wave may use, e.g. the
 * horizon-1 auxiliary problems of mld_sim_step_resolve --; on any other shape the problem is created normally and every solve takes the dense
 * path.  A solve goes the small way when, in addition, the batch is not on the LDS-resident LP path, the cost is linear, the in-kernel
 * hand-off is off, no cutoffs are set, open nodes are not recorded and time_limit == 0; a MIP start is ignored there (it is a hint), fixed
 * binaries are honoured.  The kernel reads what the dense kernel reads and answers OPTIMAL or INFEASIBLE for the same scaled, tightened
 * problem, or it DECLINES an instance (pivot or node budget spent, a pivot too small, a point that fails its own residual check, a free
 * variable resting on the artificial box); declined instances are re-solved by the dense kernel in the same call, so NODE_LIMIT, NUMERICAL
 * and UNBOUNDED are reported by it alone.  Default off.  mld_small_lds_stats tells which way the last solve went. */
#define MLD_SMALL_LDS 2

/* Solver options.  max_nodes / gap_rel / time-like limits mirror the Gurobi parameters the reference
 * forwards through **solver_kwargs (NodeLimit, MIPGap; micro_grid_control_simulation.py:232). */
typedef struct {
    double gap_abs;        /* absolute optimality tolerance (default 1e-9) */
    double gap_rel;        /* relative MIP gap (Gurobi MIPGap; default 0 = prove optimality) */
    int32_t max_nodes;     /* per instance (default 100000): nodes of the branch-and-bound tree(s) a search evaluates -- the look-ahead LPs of the dive, the
                              leaf evaluations and a MIP start are not nodes (round 4; rounds 1-3 counted every LP, which is not Gurobi's NodeLimit) */
    int32_t max_pivots;    /* per instance simplex iteration limit (default 50000) */
    int32_t cut_rounds;    /* cut rounds at the root (default -1 = max(10, min(30, binaries / 40)); 0 = no cuts) */
    int32_t cuts_per_round;/* Gomory cuts per round (default -1 = max(80, binaries / 5)) */
    int32_t max_cuts;      /* rows reserved for cuts (default -1 = max(300, rows / 4) up to 400 binaries, rows / 2 above; 0 = no cuts) */
    int32_t presolve;      /* default 6.  bit1: per-model probing-based big-M tightening (once, when the problem is created).  bit2 (round 4): per-INSTANCE
                              presolve before the root LP -- row-activity bound propagation with integer rounding on the instance's own right-hand side
                              (its x0 / omega); binaries it fixes are fixed, the implied bounds of the continuous variables are used by the rounding cuts
                              and by the test for rows that can never bind, the LP keeps the model's bounds; an instance whose rows are infeasible under
                              the bounds returns MLD_STATUS_INFEASIBLE without a pivot.  What a MIP backend's own presolve does for the
                              reference (controller_base.py:497-512 hands the instance to the solver as is).  bit0 reserved */
    int32_t n_slots;       /* solver slots = persistent workgroups (0 = auto: what is resident at once, one per CU) */
    int32_t mir_per_round; /* complemented mixed-integer rounding cuts on the original rows per cut round
                              (default -1 = 20 up to 400 binaries, binaries / 5 above; 0 = off) */
    int32_t flags;         /* MLD_F32 | MLD_SMALL_LDS (default 0, see above) */
    int32_t reserved;      /* diagnostics, default 0: the bits of mld_reserved_bit below */
    double time_limit;     /* seconds per INSTANCE on the device clock (Gurobi TimeLimit; the reference passes TimeLimit=20 with every solve,
                              examples/residential_mg_with_pv_and_dewhs/micro_grid_control_simulation.py:232, forwarded by
                              controllers/controller_base.py:509-512): the branch-and-bound of an instance ends once it has run that long, like
                              max_nodes ends it -- status MLD_STATUS_NODE_LIMIT with the incumbent and the proven bound (an instance without an
                              incumbent still gets its one rescue dive).  The clock is read between nodes, between cut rounds and, once the search has started,
                              every 128 pivots inside an LP (the root LP always runs to its end -- without it there is no answer --, and so does the rescue
                              dive), so ONE instance ends within its limit plus its root LP and a few pivots; the limit is per instance, not per call: a batch larger than
                              the number of resident workgroups takes (instances / workgroups) x time_limit at worst.  0 (default) = no limit. */
} mld_opts;

/* mld_opts.reserved: diagnostic switches.  With bits 0-5 results are the same up to rounding; only speed and traces change. */
typedef enum {
    MLD_DBG_TRACE = 1 << 0,             /* solver trace (builds with -DMLD_TRACE only) */
    MLD_DBG_REFACTOR_ALWAYS = 1 << 1,   /* refactor at every verification */
    MLD_DBG_REFACTOR_NEVER = 1 << 2,    /* never refactor */
    MLD_DBG_NO_ORDER = 1 << 3,          /* no longest-first work queue */
    MLD_DBG_KEEP_DEAD_ROWS = 1 << 4,    /* keep maintaining the rows that cannot bind under the root bounds */
    MLD_DBG_GMI_SERIAL = 1 << 5,        /* Gomory cuts one at a time (A/B of the wave-parallel round) */
    MLD_DBG_FIRST_FRACTIONAL = 1 << 6,  /* first-fractional branching instead of penalty branching */
    MLD_DBG_GEMM_VALU = 1 << 7,         /* K3 / K4 on the vector ALUs (k_rhs, k_gemm) instead of the matrix cores */
    MLD_DBG_NO_LP_LDS = 1 << 8,         /* relaxation-only batches (every binary fixed) on the dense-dictionary kernel instead of the
                                           LDS-resident revised simplex (k_lp_lds) */
    MLD_DBG_LP_LDS_K24 = 1 << 9,        /* k_lp_lds with a working-basis capacity of 24 (its overflow fall-back to the dense kernel then
                                           takes most instances) */
                                        /* (bit 10 belonged to the LDS-resident branch-and-cut experiment of rounds 2-3, removed in
                                           round 4: DESIGN section 4c) */
    MLD_DBG_LP_LDS_NO_REDO = 1 << 11,   /* leave the k_lp_lds overflow instances at status -1 instead of re-solving them (counting only) */
    MLD_DBG_NO_PRESOLVE = 1 << 12,      /* no per-instance presolve (A/B of presolve bit2 on the same problem handle) */
    MLD_DBG_NO_PERTURB = 1 << 13,       /* no anti-stalling cost perturbation in the dual simplex (A/B of round 3's change) */
    MLD_DBG_NO_LONG_STEP = 1 << 14,     /* no long-step (bound flipping) ratio test in the root LP (A/B) */
    MLD_DBG_MIR_SERIAL = 1 << 15,       /* rounding cuts built one at a time by the whole workgroup instead of a wave per cut (A/B of
                                           round 4's change) */
    MLD_DBG_NO_RESTART = 1 << 16,       /* no root restart (more cut rounds at the root of a cold instance once an incumbent leaves a gap
                                           of at most three tolerances; A/B of round 4's change) */
    MLD_DBG_LAZY_START = 1 << 17,       /* a MIP start is evaluated lazily (round 3: only when the deepening passes end without an
                                           incumbent) instead of before the root LP (A/B) */
    MLD_DBG_SUMMARY_NO_PREFETCH = 1 << 18,  /* k_log_summary (mld_sim_log_summary) stages a record without the register prefetch of the next one: the path of
                                           records wider than its registers hold, on any shape (results are bit-identical) */
    MLD_DBG_NO_SWEEP = 1 << 19,         /* no closing sweep before the in-kernel hand-off publishes a stopped search's open nodes */
    MLD_DBG_ASSERT_POSCTL = 1 << 20,    /* positive control of the assertion build (-DMLD_ASSERT): one index check fails */
    MLD_DBG_NO_PIVOT_PAIRS = 1 << 21,   /* every dual-simplex pivot updates the dictionary on its own instead of two consecutive pivots sharing
                                           one pass (A/B on the same binary: results are bit-identical, only rows_updated and speed change) */
    MLD_DBG_SIM_NO_LDS = 1 << 23,       /* k_sim_step (mld_sim_step_batch) reads x, v0, omega and y from global memory instead of staging them in LDS: the path of
                                           shapes whose staging exceeds the workgroup's LDS, on any shape (results are bit-identical) */
    MLD_DBG_CUTS_R4 = 1 << 22,          /* the wave-per-cut Gomory and c-MIR rounds as round 4 built them: one slack row / eight dictionary rows of
                                           one column chunk in flight, generic pointers (A/B on the same binary of the grouped loads and the
                                           LDS-typed views: results are bit-identical, only speed changes) */
    MLD_DBG_WALKS_SERIAL = 1 << 24,     /* k_solve's phases outside the pivot loop with one load in flight, as before the grouped walks: the row
                                           dot products of the refresh / residual check / leaf check, the thread-per-row walks over the sparse
                                           copy, the x_B update of a bound list and the row-wise screen of the c-MIR scoring (A/B on the same
                                           binary: results are bit-identical, only speed changes) */
    MLD_DBG_SMALL_PIVOT_CAP = 1 << 25,  /* k_small_milp (MLD_SMALL_LDS) with a pivot budget of 2: most instances decline and are re-solved by
                                           the dense kernel, so that the overflow route runs on any shape (the MLD_DBG_LP_LDS_K24 idea) */
    MLD_DBG_PIVOT_SYNC_R5 = 1 << 26,    /* k_solve's pivot with the block barriers it had before they were halved: six in its first half, two per
                                           SOL_NT-wide chunk of the sector and row lists (and two sums for the counts of a pair) instead of three and
                                           one exchange (A/B on the same binary: results and rows_updated are bit-identical, only speed changes) */
    MLD_DBG_SELECT_R6 = 1 << 27,        /* k_solve's choice of (row, column) as it was before its block reductions left the LDS crossbar:
                                           __shfl_down reductions with a serial combine of the waves' partials, the eligibility test of the
                                           ratio test as nested branches (A/B on the same binary: results are bit-identical, only speed changes) */
    MLD_DBG_UPDATE_R7 = 1 << 28,        /* k_solve's row updates of a pivot and of a fused pair as they were before a unit was cut down to its
                                           payload: every lane and row predicated, the entering column selected in every unit, rows handed to the
                                           waves in blocks.  Bits 26, 27 and 28 each take the dual simplex into its legacy instantiation, which
                                           holds all three earlier variants; with none of them set the loop carries only the code it runs
                                           (A/B on the same binary: results and rows_updated are bit-identical, only speed changes) */
    MLD_DBG_DEAD_WORK_R8 = 1 << 29      /* k_solve's bound changes as they were before the pass over work nobody reads: the x_B update of a bound
                                           change (one variable or a list) walks every row, the rows that are not maintained included.  The bit
                                           is read outside the pivot loop only and does not select the legacy instantiation (A/B on the same
                                           binary: results are bit-identical, only speed changes) */
} mld_reserved_bit;

/* Linear cost in tiled horizon form (the Python layer parses the reference's string-keyed atoms,
 * controllers/components/objective_atoms.py:453-521, and tiles per-step weights :118-137).
 * Each pointer is n_models x len (or NULL = zeros):
 *   lin_v  : N_tilde*nv   weight on v_tilde  (q_u, q_delta, q_z, q_mu, q_v atoms scattered into v order)
 *   lin_x  : N_tilde*nx   weight on x_tilde  (pulled back through Gamma_v: variables.py:259-265)
 *   lin_y  : N_tilde*ny   weight on y_tilde  (pulled back through L_v:     variables.py:269-275)
 * Quadratic weights (symmetric, full horizon size, NULL = none): quad_v (n x n), quad_x, quad_y --
 * cost  var' W var  (objective_atoms.py:321-331); they are assembled into P / Qx / Qw by kernel K4 and the
 * solver then runs a convex-QP relaxation (simplicial decomposition) at every branch-and-bound node. */
typedef struct {
    const double *lin_v, *lin_x, *lin_y;
    const double *quad_v, *quad_x, *quad_y;
} mld_cost;

typedef struct {
    int64_t nodes, pivots, cuts, refactors; /* totals over the batch */
    int32_t n_optimal, n_infeasible, n_node_limit, n_numerical;
    double solve_ms;                         /* device time of the solve kernel(s), HIP events */
    double rhs_ms;
} mld_stats;

/* ---- discovery / errors ------------------------------------------------------------------ */
int mld_device_count(void);
int mld_set_device(int device);
const char *mld_last_error(void);
const char *mld_version(void);
int mld_device_info(char *name, int name_len, int *n_cu, int64_t *hbm_bytes, int *lds_bytes);

/* ---- model --------------------------------------------------------------------------------
 * n_models same-shaped MLD systems  x+ = A x + B1 u + B2 d + B3 z + B4 w + b5 ; y = C x + D1 u + ... ;
 * E x + F1 u + F2 d + F3 z + F4 w + G y + Psi mu <= f5  (models/mld_model.py:456-463).
 * `mats` holds 20 pointers in the order A,B1,B2,B3,B4,b5,C,D1,D2,D3,D4,d5,E,F1,F2,F3,F4,f5,G,Psi, each
 * n_models x rows x cols row-major, NULL = zeros (the reference pads missing matrices with zeros,
 * mld_model.py:910-928; C must be passed explicitly -- the Python layer applies the C=I default :515-520). */
int mld_model_create(mld_model_t **out, const mld_dims *dims, int n_models, const double *const *mats);
/* Time-varying horizon (MldInfo / mld_numeric_tilde, models/mld_model.py:1210-1227; the time-varying branch of
 * controllers/components/mld_evolution_matrices.py:265-272): every horizon is N_tilde step models, step k acting on
 * (x(k), v(k)).  `mats` as above with n_horizons x N_tilde stacked models (horizon-major).  The handle then stands
 * for n_horizons condensed systems: mld_condense* accept only this N_tilde, and problems built on it
 * (mld_problem_create with the same N_tilde) index horizons through model_idx exactly as they index models. */
int mld_model_create_tv(mld_model_t **out, const mld_dims *dims, int n_horizons, int N_tilde, const double *const *mats);
int mld_model_destroy(mld_model_t *);

/* ---- condensing (kernels K1+K2) -----------------------------------------------------------
 * Replaces MldEvoMatrices.gen_mld_evo_matrices (controllers/components/mld_evolution_matrices.py:107-244)
 * and block_toeplitz / block_diag_dense (utils/matrix_utils.py:55-81,117-161).  Outputs (any may be
 * NULL) are n_models x the exact materialised layout of the reference's *_N_tilde matrices:
 *   Phi_x (N nx, nx)  Gamma_v (N nx, N nv)  Gamma_w (N nx, N nw)  Gamma_5 (N nx, 1)
 *   L_x   (N ny, nx)  L_v     (N ny, N nv)  L_w     (N ny, N nw)  L_5     (N ny, 1)
 *   H_x   (N nc, nx)  H_v     (N nc, N nv)  H_w     (N nc, N nw)  H_5     (N nc, 1)
 * mld_condense_device computes into device-resident buffers owned by the model (no host traffic)
 * and returns the device time of the condensing kernels; mld_condense = that + copies to host. */
int mld_condense_device(mld_model_t *, int N_tilde, int flags, double *kernel_ms);
int mld_condense(mld_model_t *, int N_tilde, int flags, double *Phi_x, double *Gamma_v, double *Gamma_w,
                 double *Gamma_5, double *L_x, double *L_v, double *L_w, double *L_5, double *H_x, double *H_v,
                 double *H_w, double *H_5);

/* fp32 materialisation (the MLD_F32 side of the condensing, SURVEY 8b / BASELINE configs[4] "fp32 condensing"): the same block
 * arithmetic in fp64 (the block products have inner dimension nx <= 15: nothing for the matrix cores), every output element
 * rounded once to fp32 on its way to HBM -- each value is the correctly rounded fp64 value, relative error <= 6e-8 -- so the
 * write stream that bounds the kernel is half as long.  Time-invariant models only. */
int mld_condense_device_f32(mld_model_t *, int N_tilde, int flags, double *kernel_ms);
int mld_condense_f32(mld_model_t *, int N_tilde, int flags, float *Phi_x, float *Gamma_v, float *Gamma_w, float *Gamma_5, float *L_x,
                     float *L_v, float *L_w, float *L_5, float *H_x, float *H_v, float *H_w, float *H_5);

/* ---- problem ------------------------------------------------------------------------------
 * Replaces MpcController.build (controllers/mpc_controller.py:76-101): condensed constraint maps
 * (on device, from the big-M-tightened model), cost pull-back (kernel K4), scaling, bounds
 * (mu >= 0, binaries in {0,1}: controllers/components/variables.py:189-243). */
/* sizeof(mld_opts) of the library build: bindings check it against their own layout before the first call that takes the struct (the struct has
 * grown: time_limit in round 3); mld_version() is bumped with every layout change. */
int mld_opts_size(void);
int mld_opts_default(mld_opts *);
int mld_problem_create(mld_problem_t **out, mld_model_t *model, int N_p, int N_tilde, const mld_cost *cost,
                       const mld_opts *opts);
int mld_problem_set_cost(mld_problem_t *, const mld_cost *cost); /* prices change every MPC step */
int mld_problem_destroy(mld_problem_t *);

/* Cost assembly (kernel K4) read-back, n_models x ...: P (n,n) q0 (n) Qx (n,nx) Qw (n,N nw); any NULL.
 * objective = 1/2 v'Pv + (q0 + Qx x_k + Qw w)'v + r(x_k,w)   (objective_atoms.py:308-331,523-532) */
int mld_cost_assemble(mld_problem_t *, double *P, double *q0, double *Qx, double *Qw);

/* ---- solve (kernels K3, K5, K6) -------------------------------------------------------------
 * Replaces the backend call `self._problem.solve(...)` (controllers/controller_base.py:509) for
 * `batch` independent instances:  model_idx[b] in [0,n_models) (NULL = all 0), x0 (batch, nx),
 * omega (batch, N_tilde*nomega) step-major, fixed_bin (batch, n_bin) with 0/1 = fixed, 255 = free
 * (NULL = all free; all fixed = relaxation-only mode).  Outputs: v_out (batch, N_tilde*nv) in the
 * reference's v_tilde order [u0;d0;z0;mu0;u1;...] (variables.py:226-241), obj_out (batch) including
 * the constant term, status_out (batch), lower_bound_out (batch, may be NULL), stats (may be NULL). */
int mld_solve_batch(mld_problem_t *, int batch, const int32_t *model_idx, const double *x0, const double *omega,
                    const uint8_t *fixed_bin, double *v_out, double *obj_out, int32_t *status_out,
                    double *lower_bound_out, mld_stats *stats_out);

/* The same in three steps so that a benchmark can time the device work with inputs resident in HBM. */
int mld_upload_batch(mld_problem_t *, int batch, const int32_t *model_idx, const double *x0, const double *omega,
                     const uint8_t *fixed_bin);

/* Extra constraint blocks of the uploaded batch.  Replaces `set_constraints(other_constraints=[gen_evo_constraints(
 * omega_scenarios_k=..., N_tilde=...), ...])` (controllers/controller_base.py:457-475 with :411-456; callers
 * examples/.../micro_grid_control_simulation.py:200-227: scenario-based and min-max controllers).  Every block
 * has the standard block's left-hand side H_v (a row prefix when its N_tilde is reduced), so the stacked system is the
 * standard one with the row-wise minimum right-hand side.  omega_cols (batch, n_cols, N_tilde*nomega): the
 * disturbance columns of all blocks (scenario columns, min / max profiles; pad reduced-horizon columns with zeros);
 * col_rows (n_cols) = number of leading constraint rows column c applies to (NULL = all rows).  Valid until the
 * next mld_upload_batch; n_cols = 0 clears. */
int mld_upload_constraint_blocks(mld_problem_t *, int n_cols, const double *omega_cols, const int32_t *col_rows);
/* The same with the state every column was generated with: the reference's gen_evo_constraints accepts an explicit x_k instead of the
 * controller's parameter (controllers/controller_base.py:411-416: `x_k = self._x_k if x_k is None else x_k`); the right-hand side of such a
 * block is H_x x_cols + H_omega omega_col + H_5.  x_cols: batch x n_cols x nx, NULL = every column uses the instance's x0. */
int mld_upload_constraint_blocks_x(mld_problem_t *, int n_cols, const double *omega_cols, const int32_t *col_rows, const double *x_cols);
int mld_solve_resident(mld_problem_t *, mld_stats *stats_out);

/* The resident solve in two halves, for callers that keep several problems busy (a fleet of independent microgrids: the reference solves
 * them one after another, controllers/controller_base.py:509).  mld_problem_use_stream gives the problem its own HIP stream;
 * mld_solve_launch queues K3 + K5/K6 on it and returns; mld_solve_finish waits, reports the statistics and learns the work-queue order.
 * While one problem's stragglers finish, the workgroups of the next problem's launch move onto the freed CUs.  Results are those of
 * mld_solve_resident, bit for bit.  (Batches on the LDS-resident kernels complete inside mld_solve_launch.) */
int mld_problem_use_stream(mld_problem_t *p);
int mld_solve_launch(mld_problem_t *p);
int mld_solve_finish(mld_problem_t *p, mld_stats *stats_out);
int mld_download_results(mld_problem_t *, double *v_out, double *obj_out, int32_t *status_out,
                         double *lower_bound_out, int32_t *nodes_out, int32_t *pivots_out);

/* Limits and tolerances of an existing problem (gap_abs, gap_rel, max_nodes, max_pivots, cut_rounds, cuts_per_round,
 * mir_per_round, reserved; negative cut fields keep the current value).  The reference passes MIPGap / NodeLimit / TimeLimit as
 * per-call **solver_kwargs of solve() (controllers/controller_base.py:491-512): they must not need a rebuild.  max_cuts,
 * n_slots and presolve shape the workspace / the tightened model and are ignored here. */
int mld_problem_set_opts(mld_problem_t *, const mld_opts *opts);
/* the options in effect, every size-scaled default (-1 fields of mld_opts_default) resolved */
int mld_problem_get_opts(mld_problem_t *, mld_opts *opts_out);

/* Receding horizon on device -- the plant update the reference performs after every solve, ControllerBase.sim_step_k ->
 * MldModel.lsim_k (controllers/controller_base.py:229-253, models/mld_model.py:647-699): for every instance of the uploaded
 * batch  x0 <- A x0 + B1 u + B2 delta + B3 z + B4 omega_0 + b5  with (u, delta, z) the step-0 slice of the last solution, and the
 * disturbance forecast moved on by one step (the first step re-enters at the end of the horizon).  The next
 * mld_solve_resident then solves the NEXT MPC step without any host traffic.  mld_download_inputs reads the current inputs. */
int mld_advance_batch(mld_problem_t *);
/* The same with the count of instances that were NOT advanced (n_skipped_out may be NULL).  Equivalence with the reference's plant step:
 * sim_step_k hands only u_k to lsim_k (controller_base.py:229-239), which re-derives delta_k, z_k (and mu_k) from (x, u, omega) by a feasibility
 * problem (_compute_aux, mld_model.py:683-686, 701-766); this entry applies the PLANNED (delta_0, z_0) instead.  The two agree when the MLD
 * model is well posed (x, u, omega determine delta, z), the plan uses no soft-constraint slack in step 0 (or delta, z do not drive the state:
 * B2 = B3 = 0, as in the example's models) and the simulated model is the controller's model.  Instances that have no usable plan -- status
 * other than OPTIMAL / NODE_LIMIT, or no incumbent -- keep their state and forecast and are counted; time-varying models
 * (mld_model_create_tv) and a batch that has not been solved since its upload are refused. */
int mld_advance_batch2(mld_problem_t *, int32_t *n_skipped_out);

/* MIP start of the resident batch (the reference calls its backend with warm_start=True, controllers/controller_base.py:493,509-512: the
 * previous values of the variables are the solver's start).  bin_start: batch x n_bin bytes, the values (0 / 1) of the binaries in the order of
 * the variable layout (step-major, controllers/components/variables.py:189-243); an instance whose first byte is 255 has no start; NULL
 * clears the start.  The start is evaluated FIRST (binaries fixed, one LP from the slack basis, verified against the original rows; the root
 * relaxation is then solved from that leaf's basis): a feasible start becomes the incumbent, the cut loop stops as soon as the bound is within
 * the gap of it, and the search -- if one is still needed -- starts around it (RINS, then the guided depth-first search).  (Round 3 evaluated it only when the first passes ended without an incumbent:
 * MLD_DBG_LAZY_START.)  Any upload / selection of new inputs clears the start. */
int mld_set_warm_start(mld_problem_t *, const uint8_t *bin_start);
/* The start built on the device from the last solution of the resident batch: shift = 0 takes the plan as it is (what warm_start=True means
 * to the reference's backend: the variables' previous values), shift = k > 0 moves it k steps towards the present and repeats its last step
 * (receding horizon: call after mld_advance_batch).  Instances without an incumbent get no start. */
int mld_warm_start_from_previous(mld_problem_t *, int shift);

/* ---- sub-tree hand-off: open nodes of a stopped search become instances of the next batch -------------------------------------
 * The reference's backend runs one branch-and-bound per solve() call to its gap (controllers/controller_base.py:509; TimeLimit 20 s in
 * the example); here a batch gives every instance ONE workgroup, so a few instances with large trees hold a launch while the other CUs
 * idle.  With recording enabled, an instance that stops at a limit inside a complete search (plain depth-first search below its
 * incumbent) returns its stack: depth, and per level the variable (index into the decision vector), its current value and a flag
 * "sibling accounted for".  Everything still open is then: for each level k with flag 0 the node {levels < k at their values, level k
 * flipped}, plus the node {all levels at their values}.  The caller uploads those nodes as instances of a new batch (same x0 / omega,
 * the node's fixings in fixed_bin, everything else 255) with the parent's incumbent value as cutoff: every CU works on the tail.
 * mld_set_cutoffs: per instance of the resident batch the objective (constant term included) that must be beaten; +inf = none, NULL
 * clears.  Under a cutoff a search that finds nothing better ends INFEASIBLE with objective +inf ("nothing better exists in this node").
 * pyhybridcontrol_amd.gpu.GpuProblem.solve_handoff drives the rounds and merges the results. */
int mld_set_cutoffs(mld_problem_t *, const double *cutoff);
int mld_record_open_nodes(mld_problem_t *, int enable);
int mld_download_open_nodes(mld_problem_t *, int32_t *depth_out, int16_t *var_out, uint8_t *val_out, uint8_t *flag_out);

/* The same hand-off INSIDE one launch (round 4): what lets ONE solve() call of the reference (controllers/controller_base.py:491-540: one instance
 * per call, its backend free to use every core on that one tree) use more than one compute unit here, and a batch keep the device busy while its
 * largest trees finish.  With it enabled the solve kernel's work queue has room for ITEMS behind the instances: an instance (or item) whose complete
 * depth-first search stops at its node limit publishes the open nodes of its stack as items -- the instance's inputs, the node's fixings, the
 * search's incumbent as cutoff -- and whichever workgroup runs out of work solves them as instances of their own (max_nodes for an instance,
 * sub_nodes for an item; a search is split at most max_gen generations deep and only while it has at most max_children open nodes; a tree that
 * cannot be split further stays MLD_STATUS_NODE_LIMIT with its incumbent and bound).  The results of a tree are merged on the device -- smallest
 * objective, on ties the node that comes first in the tree -- so mld_download_results returns per instance what an unlimited search of that
 * instance would have returned; the set of items and every item's arithmetic do not depend on which workgroup ran what, so results are
 * reproducible.  room_factor: items the queue has room for, as a multiple of the batch (at least 4096; <= 0 keeps the current value, default 2).
 * Takes effect with the next mld_upload_batch.  Not on the LDS-resident LP path (those solves run as before).  Under a quadratic cost the
 * search's closing sweep also tries the QP relaxation (its simplicial-decomposition bound) on every open sibling the LP(q) value leaves open,
 * and an item's root stops at its cutoff on the QP bound as well; a node is closed only on a proven lower bound.
 * A tree for which more than max_tree items (default 160) of ONE generation have been published keeps growing and is GIVEN UP: its remaining items are skipped and the instance
 * keeps what its own search returned (MLD_STATUS_NODE_LIMIT, incumbent, bound) -- whether that happens does not depend on the queue order.
 * mld_handoff_stats: out[0] items published by the last solve, out[1] trees given up for their size, out[2] instances that were split and are
 * still unfinished (the given-up ones included), out[3] trees given up because the queue was full (raise room_factor: the one order-dependent case). */
/* The reference's build(with_std_constraints=False) and set_constraints(std_evo_constaints=[...]) (controllers/mpc_controller.py:76-101,
 * controllers/controller_base.py:457-475): with enable = 0 the standard block -- the rows whose right-hand side comes from the batch's own
 * (x0, omega) -- is not part of the problem; only the blocks of mld_upload_constraint_blocks constrain, and a row none of them covers does not
 * exist for that solve.  Default 1. */
int mld_set_std_block(mld_problem_t *, int enable);
int mld_set_handoff(mld_problem_t *, int enable, int sub_nodes, int max_gen, int max_children, int max_tree, double room_factor);
int mld_handoff_stats(mld_problem_t *, int64_t out[4]);
/* The small-problem path (MLD_SMALL_LDS): out[0] 1 when the problem is eligible for it (flag set and the shape fits), out[1] instances the last
 * solve answered in LDS, out[2] instances it declined and the dense kernel re-solved.  out[1] = out[2] = 0 after a solve that took the dense path
 * or the LP path, and before the first solve.  MLD_ERR_NO_DEVICE without a device; MLD_ERR_INVALID for a null argument or while a launched
 * solve has not been finished. */
int mld_small_lds_stats(mld_problem_t *, int64_t out[3]);
/* How a search that reaches its node limit splits (default 0, 0 = stop and publish everything it leaves open): with donate > 0 it hands off only its
 * `donate` SHALLOWEST open nodes -- the largest open subtrees -- and goes on below them with another sub_nodes nodes, up to `rounds` times, before it
 * stops for good: the deep open nodes, which the warm dictionary closes in a few pivots each, stay where they are cheap. */
int mld_set_handoff_policy(mld_problem_t *, int donate, int rounds);
/* Scenario streaming with everything resident in HBM: the parameter update at the top of the reference's solve() (x_k and
 * omega_tilde set as cvx.Parameter values, controllers/controller_base.py:495-498; the example re-solves with new forecasts every
 * step, micro_grid_control_simulation.py:229-232) for a whole batch.  mld_stage_inputs uploads n_sets input sets of the uploaded
 * batch's size (x0_sets: n_sets x batch x nx, omega_sets: n_sets x batch x N_tilde*nomega; model_idx and fixed_bin stay those of
 * mld_upload_batch; n_sets = 0 frees them); mld_select_inputs makes set k the batch's current inputs by a device-to-device copy. */
int mld_stage_inputs(mld_problem_t *, int n_sets, const double *x0_sets, const double *omega_sets);
int mld_select_inputs(mld_problem_t *, int set);
int mld_download_inputs(mld_problem_t *, double *x0, double *omega);

/* Per-instance LINEAR cost of the resident batch (price scenarios).  The reference solves one instance per solve() call and rebuilds its
 * objective from the current tariff before every call (micro_grid_control_simulation.py:194-198,229), so every call may carry other prices;
 * here every instance of a batch may.  The cost is ADDED to the problem's cost (mld_cost of mld_problem_create / mld_problem_set_cost):
 *   lin_v (batch, N_tilde*nv)   lin_x (batch, N_tilde*nx)   lin_y (batch, N_tilde*ny)      any may be NULL = zeros
 * instance b minimises  cost_model(v) + lin_v[b]'v + lin_x[b]'x_tilde + lin_y[b]'y_tilde  -- the common part (e.g. the comfort penalty q_mu)
 * stays with the model, the scenario part (the tariff q_z) comes per instance; for replacement set the model's linear cost to zero.  Weights on
 * x_tilde / y_tilde are pulled back through the condensed maps (controllers/components/variables.py:259-275) by one batched GEMM per model on
 * the matrix cores (fp32 with MLD_F32, vector ALUs with MLD_DBG_GEMM_VALU); with lin_v alone nothing is computed.  It composes with a quadratic
 * model cost.  Valid until the next mld_upload_batch; all three NULL clears.  Survives mld_select_inputs and mld_advance_batch: the weights
 * stay, the constant term follows the current x0 / omega (it is evaluated at every launch).  The items of the in-kernel hand-off use their
 * source instance's cost; relaxation-only batches keep the LDS-resident LP (k_lp_lds reads the per-instance cost under its own column scales,
 * its overflow re-solve on the dense kernel sees the same cost); time-varying handles work like time-invariant ones (model_idx indexes
 * horizons).  Memory: batch x (n + nx + N_tilde*nomega + 1) doubles, batch x n with lin_v alone.  Runs on the problem's stream.
 * MLD_ERR_INVALID, nothing changed: no batch resident; a launched solve not finished; lin_x with nx == 0; lin_y with ny == 0. */
int mld_upload_instance_cost(mld_problem_t *, const double *lin_v, const double *lin_x, const double *lin_y);
/* Read-back, the per-instance analogue of mld_cost_assemble: q_out (batch, n) = the UNSCALED per-instance addition to the linear term, pulled
 * back to v (lin_v + Gamma_v' lin_x + L_v' lin_y); const_out (batch) = its constant term at the current x0 / omega.  Either may be NULL;
 * zeros when no per-instance cost is resident. */
int mld_download_instance_cost(mld_problem_t *, double *q_out, double *const_out);

/* Predicted state and output trajectories of the resident batch: the variables the reference builds after every solve(),
 * gen_state_output_vars (controllers/components/variables.py:246-286):
 *   x_tilde = Phi_x x_k + Gamma_v v_tilde + Gamma_omega omega_tilde + Gamma_5      (:259-265)
 *   y_tilde = L_x   x_k + L_v     v_tilde + L_omega     omega_tilde + L_5          (:269-275)
 * for every instance, as one batched GEMM per model on the matrix cores (fp32 with MLD_F32, vector ALUs with MLD_DBG_GEMM_VALU) -- the forward
 * half of the pull-back of mld_upload_instance_cost.  x_out (batch, N_tilde*nx), y_out (batch, N_tilde*ny): row-major, step-major inside a row
 * (the reference's var_N_tilde stacking); either may be NULL.
 *   v == NULL  the resident solution of the last solve.  Needs a finished solve of the CURRENT inputs: MLD_ERR_INVALID, nothing changed, when the
 *              batch was not solved since its upload / mld_select_inputs, or once mld_advance_batch has moved the inputs on (the plan belongs to
 *              inputs that are gone).  An instance without a usable plan -- the test mld_advance_batch applies when it counts skipped instances:
 *              not OPTIMAL / NODE_LIMIT with a finite objective -- gets NaN in every element of its rows.  With the in-kernel hand-off on, the
 *              instances' rows are read after the device merge.
 *   v != NULL  (batch, N_tilde*nv): the caller's plans under the batch's current x0 / omega (the `variables=` argument of the reference).  Needs
 *              only a resident batch: valid before any solve, after mld_select_inputs and after mld_advance_batch.  No NaN masking.
 * Time-varying handles work like time-invariant ones (model_idx indexes horizons).  Runs on the problem's stream and waits for that stream only.
 * MLD_ERR_INVALID: no batch resident; a launched solve not finished; x_out with nx == 0; y_out with ny == 0. */
int mld_predict_batch(mld_problem_t *, const double *v, double *x_out, double *y_out);

/* Solution quality of the resident batch: what the reference's backend reports after every solve (Gurobi's ObjVal, ConstrVio, IntVio, BoundVio
 * behind controllers/controller_base.py:509), for the resident plans or any plans of the caller, and a-posteriori scenario validation: the rows
 * evaluated under disturbance columns in the layout of gen_evo_constraints (controller_base.py:411-456) WITHOUT making them part of the problem.
 * ARITHMETIC: everything here is fp64, also on a handle created with MLD_F32 -- a certificate in fp32 certifies nothing.  Matrix cores by
 * default (k_evaluate), vector ALUs under MLD_DBG_GEMM_VALU (k_evaluate_valu, the independent cross-check).
 *   v == NULL  the resident solution of the last solve.  Needs a finished solve of the CURRENT inputs (refused like mld_predict_batch: not solved since
 *              the upload / mld_select_inputs, or mld_advance_batch has moved the inputs on).  An instance without a usable plan (not OPTIMAL /
 *              NODE_LIMIT with a finite objective) gets NaN in every floating output and -1 in constr_row_out.  With the in-kernel hand-off on, rows
 *              are read after the device merge.
 *   v != NULL  (batch, N_tilde*nv): the caller's plans under the current x0 / omega.  Needs only a resident batch; no NaN masking.
 * ROWS: always those of the ORIGINAL (un-tightened) model, condensed on the device at the problem's N_tilde on first use (as mld_rhs_batch) and
 * reused.  Residual of row i under column c:  r_i = (H_v v)_i - (H_x x_c + H_omega omega_c + H_5)_i, unscaled, in the rows' own units (Gurobi's
 * ConstrVio convention); negative = slack.
 *   n_cols == 0  the problem as posed -- the columns the next mld_solve_resident would enforce: the standard block (the batch's own x0 / omega, all
 *                rows) unless mld_set_std_block(0), plus the resident blocks of mld_upload_constraint_blocks[_x] with their col_rows / x_cols.
 *                constr_vio_out (batch) = max r_i over those columns and the rows each applies to, constr_row_out (batch) a row that attains it;
 *                -inf and -1 where no row exists (no constraint rows, or neither standard block nor blocks).
 *   n_cols > 0   the caller's validation columns, laid out as for mld_upload_constraint_blocks_x: omega_cols (batch, n_cols, N_tilde*nomega), col_rows
 *                (n_cols) leading rows a column applies to or NULL = all, x_cols (batch, n_cols, nx) or NULL = the instance's x0.  constr_vio_out and
 *                constr_row_out are (batch, n_cols), one entry per column (a column of 0 rows: -inf, -1).  The resident blocks are neither used nor changed.
 * PER INSTANCE, whatever the columns: int_vio_out (batch) = max over the binaries |v_j - rint(v_j)| (0 without binaries); bound_vio_out (batch) = the
 * largest violation of the declared bounds mu >= 0, binaries in [0, 1] (>= 0; 0 when nothing is bounded); obj_out (batch) = the value a solve would
 * report for that v at the current inputs, 1/2 v'Pv + (q0 + Qx x0 + Qw omega + q_b)'v + constant, with the cost of the last mld_problem_set_cost, a
 * resident per-instance cost in q_b and the constant, and the quadratic atoms' value at v = 0 in the constant.
 * Every output may be NULL; all NULL: success, nothing done.  Memory: batch x N_tilde*nc doubles of H_v v (twice that when nx + N_tilde*nomega > 256),
 * the results, batch x n doubles for v or a per-instance q, and the caller's columns in slices of at most 256 MB (at least one column) -- it does not
 * grow with n_cols beyond the results.  Runs on the problem's stream and waits for that stream only; nothing a later solve reads is written.
 * MLD_ERR_INVALID, nothing changed: no batch resident; a launched solve not finished; n_cols < 0; n_cols > 0 without omega_cols when nomega > 0;
 * x_cols with nx == 0; a col_rows entry outside [0, N_tilde*nc]. */
int mld_evaluate_batch(mld_problem_t *, const double *v,
                       int n_cols, const double *omega_cols, const int32_t *col_rows, const double *x_cols,
                       double *obj_out, double *constr_vio_out, int32_t *constr_row_out,
                       double *int_vio_out, double *bound_vio_out);

/* ---- resident disturbance profiles: forecasts and scenario columns by index ---------------------------------------------------------------------
 * Every disturbance window the reference hands a controller is a slice of a time series it holds once:
 *   get_omega_tilde_k_hat / _act   profile.values[start:start + N_tilde].flatten()    (examples/.../modelling/micro_grid_agents.py:236-298)
 *   get_omega_tilde_scenario       scenarios.ravel(order='F')[flat_index : flat_index + N_tilde*nomega]   (:206-232; the F-order ravel of its
 *                                  (intervals_per_day*nomega, n_days) matrix is the original (n, nomega) series, row-major)
 * and its scenario-based controllers draw 20 such columns per device at every step (examples/.../micro_grid_control_simulation.py:200-227).  A window is
 * (offset into a flat series, length): with the series resident in HBM, 20 columns of 200 doubles cross the bus as 20 integers.
 *
 * mld_upload_profiles: a flat library of lib_len doubles, owned by the PROBLEM and independent of the batch -- it survives mld_upload_batch at any batch
 * size, mld_select_inputs and mld_advance_batch.  A second call replaces it and invalidates every resident start array below; lib_len = 0 frees it;
 * mld_problem_destroy frees it.  group_width: n_groups positive widths that sum to nomega; they partition the disturbance channels 0 .. nomega-1 in order,
 * one group per fused device (NULL / n_groups = 0: one group of width nomega).  A series of group g is stored row-major (time, width_g), as the reference
 * stores a device's profile; where the series of a group begin inside the library is the caller's business (the starts say so).
 * MLD_ERR_INVALID, nothing changed: nomega == 0; widths that are not positive or do not sum to nomega; lib_len < 0; lib == NULL with lib_len > 0.
 *
 * THE WINDOW RULE.  For a start s of group g (first channel goff_g) and a step offset `step`, for k < N_tilde and channel j of group g
 *     omega[k*nomega + j] = lib[s + (step + k)*width_g + (j - goff_g)]
 * A start is valid iff s >= 0 and s + (step + N_tilde)*width_g <= lib_len.  Every start of every call is tested on the host BEFORE anything is queued --
 * the first offender is named (instance, column, group) -- and per group the largest start of a resident array is remembered on the host, so that a call
 * with start == NULL is tested without reading the device: no kernel is ever launched with an offset that has not passed.  All entry points: run on the
 * problem's stream and wait for that stream only; MLD_ERR_NO_DEVICE without a device; MLD_ERR_INVALID with nothing changed for no library, step < 0, an
 * invalid start, no batch resident, or a launched solve not finished. */
int mld_upload_profiles(mld_problem_t *, int64_t lib_len, const double *lib, int n_groups, const int32_t *group_width);
/* The forecast omega of EVERY instance of the resident batch replaced by its window; start (batch, n_groups).  x0, model_idx and fixed_bin stay.  The starts
 * stay resident: start == NULL re-uses them with another step -- how a closed loop slides every instance's window along its own series (NULL without
 * resident starts for this batch size is refused; the starts belong to a batch size and outlive an upload of the same size).
 * Between mld_advance_batch and the next solve only the forecast is touched: the batch stays advanced, the plan stays readable by
 * mld_warm_start_from_previous, and a MIP start built from it stays -- a start is a hint that is verified against the new rows.  All instances get the new
 * forecast, ALSO those the advance skipped (they kept their state, but time moves on for them too).  In every other state the call is
 * mld_select_inputs: new inputs, so the constraint blocks, the MIP start, the cutoffs and the solved state are cleared. */
int mld_forecast_from_profiles(mld_problem_t *, const int64_t *start, int step);
/* mld_upload_constraint_blocks_x with the columns gathered on the device: start (batch, n_cols, n_groups); col_rows and x_cols as there (same meaning,
 * same checks).  Fills the same resident blocks, so the solve, mld_evaluate_batch with n_cols == 0 and the in-kernel hand-off see no difference.  A column
 * with reduced col_rows still reads a FULL window: the rows beyond are never used, but the bounds test covers all N_tilde steps.  start == NULL re-uses
 * the resident column starts (same n_cols, else refused) with another step, e.g. min / max profiles sliding one step; n_cols = 0 clears the blocks. */
int mld_constraint_blocks_from_profiles(mld_problem_t *, int n_cols, const int64_t *start, int step, const int32_t *col_rows, const double *x_cols);
/* mld_evaluate_batch (above) with n_cols >= 1 validation columns gathered on the device instead of uploaded: start (batch, n_cols, n_groups), required;
 * everything else as there -- the same slices of columns, the same launches, the same results.  The resident blocks and resident starts are neither used
 * nor changed. */
int mld_evaluate_batch_profiles(mld_problem_t *, const double *v, int n_cols, const int64_t *start, int step, const int32_t *col_rows, const double *x_cols,
                                double *obj_out, double *constr_vio_out, int32_t *constr_row_out, double *int_vio_out, double *bound_vio_out);
/* Read-back of the resident constraint blocks however they got there (the counterpart of mld_download_inputs): *n_cols_out columns, omega_cols (batch,
 * n_cols, N_tilde*nomega), col_rows (n_cols; N_tilde*nc for blocks uploaded without col_rows), x_cols (batch, n_cols, nx; MLD_ERR_INVALID when the
 * resident blocks have none).  Every argument may be NULL; with all arrays NULL only the count is reported. */
int mld_download_constraint_blocks(mld_problem_t *, int32_t *n_cols_out, double *omega_cols, int32_t *col_rows, double *x_cols);

/* ---- plant step and simulation log of the resident batch -------------------------------------------------------------------------------------------
 * The step of the reference's closed loop that follows the solve: ControllerBase.sim_step_k -> MldModel.lsim_k -> MldSimLog (controllers/
 * controller_base.py:229-253, models/mld_model.py:647-699, controller_base.py:58-146), for every instance of the resident batch, without host traffic.
 * The operation is lsim_k(x_k, v_k = [u; delta; z; mu], omega_k) (mld_model.py:666-676): the WHOLE step-0 slice is given, no auxiliary is re-derived:
 *     x_k1 = A x + [B1 B2 B3] (u, delta, z) + B4 omega_k + b5                                                       (:690)
 *     y    = C x + [D1 D2 D3] (u, delta, z) + D4 omega_k + d5                                                       (:691)
 *     r    = E x + [F1 F2 F3] (u, delta, z) + F4 omega_k + G y - f5 ,   cons_i = r_i <= 1e-6                        (:692-694: the Psi mu term is zeroed)
 *     cons_vio = max_i r_i ,  cons_row = the lowest row that attains it     (-inf and -1 when nc == 0; a NaN residual wins the maximum)
 * on the ORIGINAL model's matrices, in fp64 also on an MLD_F32 handle (k_sim_step).  x_k1 is summed exactly as mld_advance_batch sums it, so an advance
 * through this entry leaves the same bits.  Under a realised disturbance `cons` says, per row, whether the PLANNED auxiliaries are still consistent with the
 * model: the test of the equivalence condition mld_advance_batch2 describes above.  Re-deriving delta / z from (x, u, omega) (lsim_k's _compute_aux) is not
 * done here but by mld_sim_step_resolve below.  The stage cost is the agent's business in the reference (sim_k.z * prices_k, examples/.../modelling/micro_grid_agents.py:753): here it is
 * written beside the record once mld_sim_log_cost_begin has armed it (resident price profiles, below).
 *
 * v0 == NULL  the step-0 slice of the resident plan.  Needs a finished solve of the current inputs that has not been advanced yet (refused exactly where
 *             mld_predict_batch(v = NULL) is refused); rows are read after the hand-off's device merge.  An instance without a usable plan (not OPTIMAL /
 *             NODE_LIMIT with a finite objective) is NOT advanced (it keeps state and forecast) and is counted in n_skipped_out; its outputs and its record
 *             have NaN in v, y, x_k1 and cons_vio, 0 in cons and -1 in cons_row; x, omega, obj, lower_bound, status and nodes are recorded as they are.
 * v0 != NULL  (batch, nv): the caller's step inputs (a rule-based baseline, another controller).  Needs only a resident batch; no masking, every instance
 *             advances, n_skipped_out = 0.  The record carries obj = lower_bound = NaN, status = -1, nodes = 0.
 * omega_k     the forecast's step 0, or with MLD_SIM_ACTUAL one element run of the profile library (mld_upload_profiles): the window rule with ONE step,
 *             omega_k[j] = lib[s + step*width_g + (j - goff_g)] for channel j of group g with start s.  act_start (batch, n_groups) stays resident in an
 *             array of its own (separate from the forecast and column starts); NULL re-uses it with another step.  Every start is tested on the host before
 *             anything is queued (s >= 0, s + (step + 1)*width_g <= lib_len; per group the largest resident start is remembered), the first offender is
 *             named by instance and group; mld_upload_profiles invalidates the resident starts.
 * MLD_SIM_ADVANCE  x0 <- x_k1 and the forecast rotated by one step: everything mld_advance_batch2 does.  With the resident plan the handle ends in the state
 *             mld_advance_batch2 leaves (advanced; constraint blocks, MIP start and cutoffs cleared: mld_warm_start_from_previous and
 *             mld_forecast_from_profiles(NULL, step + 1) work as after it).  With the caller's v0 it ends as after mld_select_inputs (new inputs: blocks, MIP
 *             start, cutoffs and solved state cleared).  Without the flag nothing a later solve reads is written: a what-if under another realised value.
 * MLD_SIM_LOG  this step's record is appended to the resident log, slot n_logged, which then increments.
 * Outputs (any may be NULL): x_k1_out (batch, nx), y_out (batch, ny), cons_out (batch, nc) bytes 0 / 1, cons_vio_out (batch), cons_row_out (batch).
 *
 * THE LOG.  mld_sim_log_begin(capacity) allocates `capacity` records of the resident batch and resets the count (a log held before is replaced; 0 frees):
 * capacity x batch x ((2 nx + nv + ny + nomega + 3) doubles + nc bytes + 3 ints), the product in size_t; an allocation failure reports an error and changes
 * nothing.  The log belongs to the resident batch: mld_upload_batch discards it, mld_problem_destroy frees it.  mld_download_sim_log copies records
 * [first, first + count) into arrays (count, batch, width), any NULL: x, v, y, omega (the omega_k used), x_k1, cons, cons_vio, cons_row as above, and the
 * solve's obj, lower_bound, status, nodes as mld_download_results reports them.
 *
 * Runs on the problem's stream; it waits for that stream only, and only where it has to: for the caller's arrays (v0, act_start), the skip count and the
 * requested outputs (and after MLD_SIM_ADVANCE on a stream made by mld_problem_use_stream, which the copies of the other entry points do not order against).
 * MLD_ERR_NO_DEVICE without a device.  MLD_ERR_INVALID, nothing changed: no batch resident; a launched solve not finished; a time-varying handle (as
 * mld_advance_batch); unknown flag bits; step < 0; MLD_SIM_ACTUAL without a library, with nomega == 0, or with an invalid or missing start (act_start without
 * the flag too); MLD_SIM_LOG without a begun log or with a full one; a download range outside [0, n_logged]. */
#define MLD_SIM_ADVANCE 1   /* x0 <- x_k1, forecast rotated by one step: everything mld_advance_batch2 does */
#define MLD_SIM_ACTUAL  2   /* omega_k from the profile library instead of the forecast's step 0 */
#define MLD_SIM_LOG     4   /* append this step's record to the resident log */
int mld_sim_log_begin(mld_problem_t *, int capacity);
int mld_sim_log_count(mld_problem_t *, int32_t *n_logged, int32_t *capacity);
int mld_sim_step_batch(mld_problem_t *, const double *v0, const int64_t *act_start, int step, int flags,
                       double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out, int32_t *n_skipped_out);
int mld_download_sim_log(mld_problem_t *, int first, int count,
                         double *x, double *v, double *y, double *omega, double *x_k1, uint8_t *cons, double *cons_vio, int32_t *cons_row,
                         double *obj, double *lower_bound, int32_t *status, int32_t *nodes);

/* ---- the plant step with the auxiliaries re-derived ------------------------------------------------------------------------------------------------
 * What the reference's closed loop does: ControllerBase.sim_step_k (controllers/controller_base.py:229-253) calls lsim_k(x_k=, u_k=, omega_k=) with u ONLY;
 * MldModel.lsim_k (models/mld_model.py:683-686) then calls _compute_aux (:701-766), a small feasibility MIP for delta, z, mu under the REALISED omega_k, and
 * only then forms x_k1, y and cons.  mld_sim_step_resolve is that step for every instance of the resident batch without host traffic: under a realised
 * disturbance the auxiliaries follow the model (for the microgrid models z = delta y is the grid power that occurred, not the forecast's).
 *
 * aux         the resolver's handle, passed with every call (no pointer is kept): a problem over the FOLDED models -- u moved into the disturbance channel,
 *             omega' = [omega; u], so nu = 0 and nomega' = nomega + nu; every other dimension and n_models as this problem's -- with N_tilde = 1 and the cost
 *             sum(mu) (aux_resolve.BatchAuxResolver builds it).  Of the feasible points the reference may return, the one with the least total slack is
 *             taken.  aux == NULL is required iff ndelta + nz + nmu == 0; the step then equals mld_sim_step_batch with v0 = u.
 * u0 == NULL  the first nu entries of the resident plan's row; refused where mld_sim_step_batch(v0 = NULL) is refused.  An instance is ATTEMPTED iff its plan
 *             is usable.  u0 != NULL: (batch, nu), the caller's inputs, no plan needed, every instance attempted; tested for finiteness on the host.
 * omega_k, act_start, step, flags: exactly as mld_sim_step_batch (the resident actual starts are shared with it).
 * One call:   k_aux_inputs writes the resolver's inputs on the device, x0' = x and omega' = [omega_k; u] (u = 0 for an instance that is not attempted); the
 *             resolver's resident batch (size, model_idx, RHS groups) is laid out by the call whenever it is not this batch's -- another size, or either handle
 *             uploaded since --, which costs one device-to-host copy of model_idx and the upload path; the steps in between move nothing over PCIe but what
 *             the caller passes or asks for (the solve path's own bookkeeping aside).  The resolver solves (its inputs count as replaced, as after
 *             mld_select_inputs).  k_aux_merge builds v0 = [u; delta; z; mu] per instance and its usable flag: attempted AND the resolver ended OPTIMAL or at
 *             NODE_LIMIT with a finite objective (a feasible point, all the reference asks for).  k_sim_step steps on v0 with that flag as mask: an unusable
 *             instance is treated as an instance without a usable plan is by mld_sim_step_batch -- not advanced, counted in n_skipped_out, NaN / 0 / -1 in
 *             its outputs and NaN in the record's v (the reference returns NaN auxiliaries and hence a NaN x_k1 there, :757-763).  The host waits between
 *             the three phases; the call is host-synchronous.
 * Outputs     as mld_sim_step_batch, plus v0_out (batch, nv) the resolved slices (NaN rows where unusable) and aux_status_out (batch) the resolver's status
 *             per instance, -1 where it was not attempted (0 with aux == NULL).
 * MLD_SIM_ADVANCE  as mld_sim_step_batch: with u0 == NULL the handle ends `advanced`, with the caller's u0 as after mld_select_inputs.
 * MLD_SIM_LOG  the usual record, its v the resolved slice, obj / lower_bound / status / nodes the plan's (NaN / NaN / -1 / 0 with u0 given); and aux_status
 *             in an int array (capacity, batch) that the first resolving step that logs allocates, filled with -2 = "not resolved"; mld_sim_log_begin
 *             discards it.  mld_download_sim_log_aux copies records [first, first + count): -2 for records mld_sim_step_batch wrote.
 * MLD_ERR_INVALID before anything is queued, nothing changed on either handle: everything mld_sim_step_batch refuses; aux == the problem itself; aux with a
 * launched solve, with N_tilde != 1, time-varying, with the in-kernel hand-off on, or whose dimensions are not the fold of this problem's; aux NULL / not
 * NULL against the rule above; a u0 that is not finite.  An error in a later phase leaves this problem's inputs, log count and actual starts as they were. */
int mld_sim_step_resolve(mld_problem_t *, mld_problem_t *aux, const double *u0, const int64_t *act_start, int step, int flags,
                         double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out,
                         double *v0_out, int32_t *aux_status_out, int32_t *n_skipped_out);
int mld_download_sim_log_aux(mld_problem_t *, int first, int count, int32_t *aux_status);

/* ---- open-loop rollout of plans under realised disturbances ------------------------------------------------------------------------------------------
 * The question a scenario-based controller asks after every solve: what does the hybrid plant do over the next K steps if this plan is applied and the
 * disturbance turns out to be realisation c?  The reference answers with MldModel.lsim, or lsim_k in a loop (models/mld_model.py:543-642, 647-699), which
 * calls _compute_aux (:701-766) -- one feasibility MIP -- per device, step and realisation.  mld_rollout_batch runs batch x S trajectories of K steps in
 * ONE launch (k_rollout): a 64-lane wave per trajectory (instance b, realisation c), t = b S + c; per step the resolver's right-hand side, its auxiliary
 * problem solved in the wave's LDS by the solver of MLD_SMALL_LDS (min sum(mu)), then x_{k+1}, y_k and the hard-constraint residuals with the sums of
 * mld_sim_step_batch (fp64 on the ORIGINAL matrices, the Psi mu term zeroed, a NaN residual wins the maximum, ties to the lower row).
 *
 * aux         the resolver's handle of mld_sim_step_resolve (the folded models, N_tilde = 1), created with MLD_SMALL_LDS and eligible for that path; NULL is
 *             required iff ndelta + nz + nmu == 0 (the rollout is then a plain lsim).  Only its per-model data is read; nothing on it changes.
 * u_seq       (batch, K, nu), or NULL: the inputs of the resident plan (K <= N_tilde; needs a finished solve that has not been advanced); an instance
 *             without a usable plan is not attempted.
 * omega_seq   (batch, S, K, nomega) realised disturbances, or start (batch, S, n_groups) offsets into the resident profile library with the window rule
 *             s >= 0, s + (step + K) width_g <= lib_len: exactly one of the two (neither when nomega == 0).
 * cost_w      (cost_rows, K, nv) weights of cost = sum_k w_k . v_k, a row per model (cost_rows == n_models) or per instance (== batch), or NULL.
 * Outputs     any may be NULL.  Per step: x_out (batch, S, K + 1, nx) with x_out[.., 0, :] = x0, v_out (batch, S, K, nv) = [u; delta; z; mu],
 *             y_out (.., ny), cons_vio_out / cons_row_out (batch, S, K).  Per trajectory (batch, S): cost_out, mu_total_out = sum_k sum(mu_k), worst_vio_out
 *             = the largest cons_vio over the steps (a NaN wins, the earliest step of equals) with worst_step_out, steps_done_out and end_status_out:
 *                0  complete;
 *                1  the auxiliary problem of step steps_done has no feasible point: that step and the later ones hold NaN / -1, as the reference returns
 *                   NaN auxiliaries there (:757-763);
 *                2  the LDS solver declined at step steps_done (pivot or node budget, a pivot too small ...): the state it stopped at is in
 *                   x_out[.., steps_done, :], the rest NaN / -1 -- there is no dense fall-back in the kernel; finish such a trajectory stepwise
 *                   (GpuProblem.rollout does, with the resolver's own solve);
 *               -1  not attempted (u_seq == NULL and no usable plan): every output NaN / -1, steps_done 0.
 *             The summaries of a trajectory that did not end 0 are NaN / -1.  stats: trajectories, then those that ended 0, 1 and 2.
 * The call reads the handle's current x0 and writes nothing a solve reads: inputs, plan, MIP start, log and resident starts are unchanged (the what-if of
 * mld_sim_step_batch without MLD_SIM_ADVANCE).  MLD_DBG_SMALL_PIVOT_CAP on the resolver's options caps the pivots as in a solve: every trajectory then
 * ends 2 at step 0.  Host-synchronous.
 * MLD_ERR_INVALID before anything is queued, nothing changed: no resident batch; a time-varying model; K < 1, S < 1; K > N_tilde, an unsolved or an
 * advanced batch with u_seq == NULL; aux NULL / not NULL against the rule above, aux == the problem itself, with a launched solve, N_tilde != 1,
 * time-varying, with the hand-off on, not the fold of this problem's models, not on the small-problem path (the message points to mld_sim_step_resolve),
 * with a quadratic / per-instance cost or fixed binaries; a staging that does not fit; both or neither of omega_seq / start; no library or a start
 * outside it; cost_rows that is neither n_models nor batch; a u_seq, omega_seq or cost_w that is not finite. */
int mld_rollout_batch(mld_problem_t *p, mld_problem_t *aux, int K, int S, const double *u_seq, const double *omega_seq, const int64_t *start, int step,
                      const double *cost_w, int cost_rows, double *x_out, double *v_out, double *y_out, double *cons_vio_out, int32_t *cons_row_out,
                      double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out,
                      int32_t *end_status_out, int64_t stats[4]);

/* ---- rule-based feedback (thermostat) policies ------------------------------------------------------------------------------------------------------
 * The reference's simulation campaign quotes every saving of its MPC variants against `thermo`, DewhTheromstatController (examples/
 * residential_mg_with_pv_and_dewhs/controllers/theromstat_control.py:38-64): a hysteresis rule u_k = f(x_k, u_{k-1}) per tank, stepped through sim_step_k
 * (controllers/controller_base.py:229-253) like every other controller.  Here the rule is data per model m and input channel j:
 *     sel (n_models, nu, nx) selector rows; on_at, off_at, u_on, u_off (n_models, nu); mode (n_models, nu): 0 the channel is passed through -- its value
 *     comes from u_seq / u0 / the resident plan exactly as without a policy --, 1 it is ruled.
 * For a ruled channel, with s = sum_i sel[m,j,i] x[i] (fp64, i ascending), in this order (:53-58):
 *     s <= on_at -> u_on;   s >= off_at -> u_off;   u_prev[j] == u_on -> u_on (exact equality, the reference's `== 1`);   otherwise u_off.
 * A NaN s falls through to the last two lines, as in the reference; on_at <= off_at is required, and at equality the first line wins.
 *
 * mld_upload_policy: the tables, n_models rows each, owned by the PROBLEM and independent of the batch, like the profile library; sel == NULL removes the
 * policy.  Validated on the host: every value finite, on_at <= off_at, mode 0 or 1 (MLD_ERR_INVALID, the resident policy stays).  A new policy resets the
 * resident policy state.
 * mld_set_policy_state / mld_download_policy_state: the resident u_prev (batch, nu), the input applied before the next step.  u_prev == NULL resets every
 * ruled channel to its model's u_off (a passed-through one to 0): the state after any mld_upload_batch -- the reference's first step has no previous
 * record, so `u_k_neg1 == 1` is false (:57).  MLD_ERR_INVALID: no resident batch, no policy, a u_prev that is not finite.
 *
 * mld_rollout_policy: mld_rollout_batch with the rule in the loop (kernel k_rollout_policy, the second instantiation of k_rollout's body) -- the K-step,
 * S-realisation Monte-Carlo of the baseline in one launch, where the reference runs lsim_k per device, step and realisation.  Trajectories, endings,
 * statuses and outputs mean what they mean for mld_rollout_batch.  At step k the ruled channels take the rule's value from the trajectory's own x_k and its
 * own u_{k-1}; before step 0 that is u_prev (batch, nu), or, if NULL, the resident policy state.  u_seq supplies the passed-through channels (its ruled
 * channels are ignored but must be finite); u_seq == NULL with every channel ruled needs no plan and attempts every instance, with any passed-through
 * channel it takes those channels from the resident plan under mld_rollout_batch's rules (K <= N_tilde, an unusable plan: -1).  switches_out (batch, S)
 * int32 counts the (step, ruled channel) pairs with u_k[j] != u_{k-1}[j], -1 unless the trajectory ended 0.  The call changes nothing on the handle, the
 * resident policy state included.  MLD_ERR_INVALID before anything is queued: everything mld_rollout_batch refuses; no policy; a u_prev that is not finite.
 *
 * mld_sim_step_policy: ONE resolving plant step, mld_sim_step_resolve's own phases behind a kernel that writes u (k_policy_inputs, threads on (instance,
 * channel)) from the handle's current x0, the resident u_prev and the tables into the buffer the step reads its u0 from.  u0 supplies the passed-through
 * channels; NULL follows the rollout's rules: the resident plan for them, or no plan needed when every channel is ruled.  With MLD_SIM_ADVANCE the resident
 * u_prev of every ADVANCED instance becomes the u applied (skipped instances keep theirs); without it the state is not written (the what-if).  aux == NULL
 * for models without auxiliaries: the step is then mld_sim_step_batch with v0 = u.  With MLD_SIM_LOG the record is what the resolving step writes.
 * Outputs and refusals as mld_sim_step_resolve, plus: no policy uploaded. */
int mld_upload_policy(mld_problem_t *p, const double *sel, const double *on_at, const double *off_at, const double *u_on, const double *u_off, const int32_t *mode);
int mld_set_policy_state(mld_problem_t *p, const double *u_prev);
int mld_download_policy_state(mld_problem_t *p, double *u_prev_out);
int mld_rollout_policy(mld_problem_t *p, mld_problem_t *aux, int K, int S, const double *u_seq, const double *u_prev, const double *omega_seq, const int64_t *start,
                       int step, const double *cost_w, int cost_rows, double *x_out, double *v_out, double *y_out, double *cons_vio_out, int32_t *cons_row_out,
                       double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out,
                       int32_t *end_status_out, int32_t *switches_out, int64_t stats[4]);
int mld_sim_step_policy(mld_problem_t *p, mld_problem_t *aux, const double *u0, const int64_t *act_start, int step, int flags,
                        double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out,
                        double *v0_out, int32_t *aux_status_out, int32_t *n_skipped_out);

/* ---- fallback inputs for instances without a usable plan ----------------------------------------------------------------------------------------------
 * mld_advance_batch[2], mld_sim_step_batch(v0 = NULL) and mld_sim_step_resolve(u0 = NULL) do not advance an instance whose solve left no usable plan (status
 * other than OPTIMAL / NODE_LIMIT, or no finite objective): its plant keeps its state while the clock and the profile windows move on for every instance.
 * The reference never freezes a plant: solve_grid_mpc catches the solver's error, warns "Using last solution, will not be optimal" and goes on (examples/
 * residential_mg_with_pv_and_dewhs/modelling/micro_grid_agents.py:728-735), and sim_step_k steps the plant with whatever variables_k.u holds (controllers/
 * controller_base.py:229-253).  mld_sim_step_fallback is the resolving step with the source of u chosen per instance on the device.
 *
 * Plan memory  resident and opt-in (mld_plan_memory), owned by the resident batch like the policy state: mem_u (batch, N_tilde, nu) fp64 and mem_age (batch)
 *             int32.  age = -1: nothing remembered; age = a >= 1: the remembered plan was made a advancing steps ago, so its row a is the input it planned for
 *             NOW; age = N_tilde: exhausted.  (The reference re-applies the stale plan's step-0 input; row a is the receding-horizon-consistent choice.)
 * Source of u  at a fallback step, the first that applies, per instance b:
 *                0  PLAN     the plan is usable                                      the first nu entries of the resident plan's row
 *                1  MEMORY   MLD_FB_MEMORY in fb and 1 <= age[b] <= N_tilde - 1      mem_u[b, age[b], :]
 *                2  POLICY   MLD_FB_POLICY in fb                                     the resident policy's rule on the handle's current x0[b] and the resident
 *                                                                                    u_prev[b] (the arithmetic and branch order of mld_sim_step_policy)
 *               -1  NONE     none of the above                                       the instance is not attempted, exactly as an instance without a usable
 *                                                                                    plan is by mld_sim_step_resolve(u0 = NULL)
 *             An instance is attempted iff its source is >= 0.  From there on the step is mld_sim_step_resolve's own phases, unchanged: k_aux_inputs, the
 *             resolver's solve, k_aux_merge, k_sim_step under the merged usable mask.  With fb == 0 the call is mld_sim_step_resolve(u0 = NULL) bit for bit,
 *             and u_source is 0 or -1.
 * Commit      only with MLD_SIM_ADVANCE, after the step has been queued without an error.  An enabled memory (whether or not fb names it): source 0 ->
 *             mem_u[b, k, :] = the plan's u of step k for all k and age[b] = 1, whether or not the instance advanced; any other source with age[b] >= 1 ->
 *             age[b] = min(age[b] + 1, N_tilde); age -1 stays -1.  A resident policy (whether or not fb names it): u_prev of every ADVANCED instance becomes
 *             the u applied, whatever its source, so the rule's hysteresis state is right when it takes over.  Without MLD_SIM_ADVANCE nothing is written:
 *             memory, u_prev and inputs all stay.  After an advancing step the handle is as after mld_sim_step_resolve(u0 = NULL): `advanced`.
 * Validity    the memory is valid only along an unbroken chain of advancing fallback steps.  Every age goes back to -1 with mld_upload_batch,
 *             mld_select_inputs, any call that replaces x0, and an advance through any other entry point (mld_advance_batch[2], mld_sim_step_batch,
 *             mld_sim_step_resolve, mld_sim_step_policy); not with mld_forecast_from_profiles, a solve, mld_problem_set_cost or mld_upload_instance_cost.
 * Outputs     as mld_sim_step_resolve, plus u_source_out (batch).
 * MLD_SIM_LOG  the usual resolving record -- obj / lower_bound / status / nodes the plan's as they are --, and u_source in an int array (capacity, batch) that
 *             the first fallback step that logs allocates, filled with -2 = "written by another entry point"; mld_sim_log_begin discards it.
 *             mld_download_sim_log_source copies records [first, first + count).
 * mld_plan_memory: enable != 0 allocates the memory and empties it (every age -1), 0 frees it; needs a resident batch.  mld_set_plan_memory seeds or restores
 * it -- u (batch, N_tilde, nu) finite, age (batch) in {-1, 1 .. N_tilde}, either may be NULL (kept) --, mld_download_plan_memory reads it.
 * MLD_ERR_INVALID before anything is queued, nothing changed on either handle: everything mld_sim_step_resolve(u0 = NULL) refuses (an unsolved or already
 * advanced batch, a time-varying handle, a launched solve, the rules for aux); unknown fb bits; MLD_FB_MEMORY without an enabled memory; MLD_FB_POLICY
 * without a resident policy or with one that passes a channel through (the message says why); nu == 0. */
#define MLD_FB_MEMORY 1
#define MLD_FB_POLICY 2
int mld_plan_memory(mld_problem_t *, int enable);
int mld_set_plan_memory(mld_problem_t *, const double *u, const int32_t *age);
int mld_download_plan_memory(mld_problem_t *, double *u_out, int32_t *age_out);
int mld_sim_step_fallback(mld_problem_t *, mld_problem_t *aux, int fb, const int64_t *act_start, int step, int flags,
                          double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out,
                          double *v0_out, int32_t *aux_status_out, int32_t *u_source_out, int32_t *n_skipped_out);
int mld_download_sim_log_source(mld_problem_t *, int first, int count, int32_t *u_source);

/* ---- applying a selection on the device ------------------------------------------------------------------------------------------------------------------
 * mld_rollout_select and mld_rollout_select_policy (below) answer "which candidate should be applied now"; applying the answer through
 * mld_sim_step_resolve(u0 = the downloaded u0_choice) sends u0 down and up again on every step, empties the plan memory (the advance is another entry
 * point's), leaves the resident policy's u_prev where it was, logs u_source -2, and attempts an instance without an admissible candidate with a NaN row.
 * mld_sim_step_selected is the resolving step with the selection as the FIRST source of u, in place of the plan, and the memory, the policy state and the
 * log consistent with what was applied.
 *
 * Kept selection  owned by the resident batch: choice (batch) int32, -1 = none; policy (batch) int32, the policy index of the pick, -1 for a plan or sequence
 *             pick or no pick; u (batch, K, nu) fp64, exactly what the select call returns as u_choice -- a policy pick has the rule's step 0 in row 0 and
 *             NaN behind it, no choice is all NaN --; and K.  mld_keep_selection(p, enable) is sticky, like mld_set_rollout_completion: while it is on, every
 *             successful mld_rollout_select / mld_rollout_select_policy on p leaves its selection there, copied device to device from the call's temporaries
 *             behind k_plan_select / k_select_inputs on the same stream, and swapped in only when the call has succeeded (a call that fails leaves the
 *             previous one).  Off (the default): nothing is allocated, no copy is queued.  enable = 0 frees the buffers.
 *             mld_set_selection puts a caller's own selection there (a filter of the caller's, or the instances a host completion corrected), staged and
 *             swapped in as mld_set_plan_memory does; policy == NULL: every pick is a sequence.  mld_download_selection reads it: K, the arrays (any NULL)
 *             and valid (1 / 0).
 * Validity    the selection is stamped with the batch and the inputs it was made for and is valid while both are unchanged -- the plan memory's rule:
 *             mld_forecast_from_profiles, a solve, mld_problem_set_cost and mld_upload_instance_cost keep it; mld_upload_batch, mld_select_inputs,
 *             mld_advance_batch[2] and an advancing step of any entry point (this one included: the selection is consumed) end it.
 * Source of u  at a selected step, the first that applies, per instance b:
 *                3  SELECTED  choice[b] >= 0                                         u[b, 0, :] of the kept selection
 *                1  MEMORY    MLD_FB_MEMORY in fb and 1 <= age[b] <= N_tilde - 1     mem_u[b, age[b], :]                    (mld_sim_step_fallback's rule)
 *                2  POLICY    MLD_FB_POLICY in fb                                    the resident policy's rule             (mld_sim_step_fallback's rule)
 *               -1  NONE      none of the above                                      not attempted
 *             The resident plan is deliberately NOT a source: either the filter judged it (plan_first) or the caller left it out, so an instance without an
 *             admissible candidate goes to the memory or the policy.  From there on the step is mld_sim_step_resolve's own phases, unchanged.  No channel of
 *             u is the plan's, so no solved plan is needed, the record's obj / lower_bound / status / nodes are those of mld_sim_step_resolve(u0), and after
 *             an advancing step the handle is as after mld_sim_step_resolve(u0): new inputs, not solved.
 * Commit      only with MLD_SIM_ADVANCE, after the step has been queued without an error.  An enabled memory (whether or not fb names it): an instance of
 *             source 3 with a plan or sequence pick (policy[b] < 0) and K == N_tilde is remembered -- mem_u[b] = u[b], age[b] = 1, read from the source, not
 *             from the advanced mask, as mld_sim_step_fallback reads it --; every other instance ages as a non-plan source does.  The memory's rows are the
 *             time slots of a full horizon, so with K != N_tilde nothing is remembered.  The memory follows the advance: it survives the step.  A resident
 *             policy: u_prev of every ADVANCED instance becomes the u applied.  Without MLD_SIM_ADVANCE nothing is written and the selection stays valid.
 * Outputs     as mld_sim_step_fallback (u_source 3 / 1 / 2 / -1), plus pick_out (batch): choice[b] where the source is 3, -1 elsewhere.
 * MLD_SIM_LOG  the record of mld_sim_step_resolve(u0), u_source in the array of mld_download_sim_log_source (3 is new there; mld_sim_log_summary's n_source
 *             keeps its three columns, a record of source 3 counts in none), and pick in an int array (capacity, batch) beside it, -2 for the records of
 *             other entry points: mld_download_sim_log_pick copies records [first, first + count).
 * MLD_ERR_INVALID before anything is queued, nothing changed on either handle: no kept selection; a stale one (the message says what ended it); unknown fb
 * bits and everything mld_sim_step_fallback refuses for its bits; everything mld_sim_step_resolve(u0) refuses.  mld_set_selection names the instance: K < 1;
 * choice < -1; policy < -1, or >= 0 without a choice; where choice[b] >= 0, u[b, 0, :] not finite, and for a plan or sequence pick (policy[b] < 0) any row. */
int mld_keep_selection(mld_problem_t *p, int enable);
int mld_set_selection(mld_problem_t *p, int K, const int32_t *choice, const int32_t *policy, const double *u);
int mld_download_selection(mld_problem_t *p, int32_t *K_out, int32_t *choice, int32_t *policy, double *u, int32_t *valid_out);
int mld_sim_step_selected(mld_problem_t *, mld_problem_t *aux, int fb, const int64_t *act_start, int step, int flags,
                          double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out,
                          double *v0_out, int32_t *aux_status_out, int32_t *u_source_out, int32_t *n_skipped_out, int32_t *pick_out);
int mld_download_sim_log_pick(mld_problem_t *, int first, int count, int32_t *pick);

/* ---- MIP start from a baseline rollout ------------------------------------------------------------------------------------------------------------------
 * mld_warm_start_from_previous gives an instance without a usable plan no start (255), and so does the first solve after an upload: exactly the hard
 * instances enter the search cold.  The reference hands its backend whatever values the variables hold (warm_start=True, controllers/controller_base.py:493,
 * 509-512).  mld_warm_start_from_rollout builds the start ON THE DEVICE from a rollout of the handle's current x0 under the RESIDENT FORECAST (the omega the
 * next solve plans against: batch x N_tilde x nomega, step-major, read where it lies), K = N_tilde steps, one trajectory per instance:
 *   policy = 1   the resident rule-based policy in closed loop (k_rollout_policy) -- a thermostat keeps every tank inside its band; where its plan is feasible
 *                for the MPC's rows (it need not be for every instance: the solver verifies a start like any other, and one that is not feasible gives no
 *                incumbent), the start, evaluated first as mld_set_warm_start describes (lazily with a quadratic cost or under MLD_DBG_LAZY_START), is
 *                an incumbent no worse than the baseline.  u_prev (batch, nu) or
 *                NULL = the resident policy state, which the call does not write; u_seq (batch, N_tilde, nu) supplies the passed-through channels under
 *                mld_rollout_policy's rules (NULL with every channel ruled needs no plan).
 *   policy = 0   the caller's u_seq (batch, N_tilde, nu), required (k_rollout) -- another controller's plan as the start of this one; the auxiliaries are
 *                re-derived for THIS handle's forecast.
 * The start (k_warm_from_rollout, threads on (instance, binary)): binary k of instance b, bins[k] = step nv + pos, takes v[b, step, pos] > 0.5 ? 1 : 0 of the
 * rolled-out v, which is a device temporary and never downloaded.  source_out (batch) int32, or NULL:
 *      1   start written from the rollout
 *      0   existing start kept: MLD_START_KEEP in flags, a start is resident, and the row's first byte is not 255
 *     -1   the auxiliary problem of some step has no feasible point              } the whole row 255 = no start
 *     -2   the LDS solver declined (this entry has no host completion)           }
 *     -3   not attempted: a passed-through channel needed the plan and there is none usable
 * Without MLD_START_KEEP, or with no start resident, every row is written.  stats (or NULL): trajectories, rows written, kept, none.
 * Afterwards a start is set (as after mld_set_warm_start), unless the problem has no binary: then the call, once every check below has passed, returns
 * MLD_OK, rolls nothing and writes neither output.  Nothing else changes on the handle -- inputs, plan, solved / advanced, cutoffs, log, policy state, plan memory, resident starts -- and nothing
 * on aux.  The start is formed from fp64 buffers on every handle (the forecast and the rollout are fp64 also under MLD_F32).
 * MLD_ERR_INVALID before anything is queued, the resident start as it was: everything mld_rollout_batch / mld_rollout_policy refuse (a time-varying model, a
 * resolver off the small-problem path, a u_seq or u_prev that is not finite, no policy, ...); policy = 0 with u_seq == NULL; u_prev with policy = 0; unknown
 * flag bits; a launched solve that has not been finished. */
#define MLD_START_KEEP 1   /* instances that already have a start keep it */
int mld_warm_start_from_rollout(mld_problem_t *p, mld_problem_t *aux, int policy, const double *u_seq, const double *u_prev,
                                int flags, int32_t *source_out, int64_t stats[4]);

/* ---- resident price profiles: tariff windows into the cost, stage cost in the log -----------------------------------------------------------------------
 * Every solve of the reference's closed loop starts from a price window and every plant step ends in a price: GridAgentMpc.get_price_tilde_k(k) cuts
 * price_profile.values[start:start + N_tilde] out of a series it holds once (examples/.../modelling/micro_grid_agents.py:563-606), sim_mpc turns the window
 * into the objective before every solve() (micro_grid_control_simulation.py:186-198: q_z = prices_tilde, q_mu = sum(prices_tilde) * P_h_Nom * mult), and
 * sim_step_k multiplies the realised import by the price of the step (micro_grid_agents.py:746-755), summed into total_cost_struct (:239-243).
 *
 * mld_upload_prices: a flat library of lib_len doubles, owned by the PROBLEM like the disturbance library and separate from it (prices are not disturbance
 * channels and have no groups) -- it survives mld_upload_batch, mld_select_inputs and the advances.  n_chan >= 1 price channels; a series is row-major
 * (time, n_chan), as price_profile.values is.  A second call replaces it, invalidates the resident price starts and disarms a stage cost; the tables below
 * stay unless n_chan changes (it shapes them).  lib_len = 0 frees the library and everything that hangs on it; mld_problem_destroy frees it.
 * MLD_ERR_INVALID, nothing changed: lib_len < 0; lib == NULL with lib_len > 0; n_chan < 1; (N_tilde + 1) x n_chan above 6144 doubles (the LDS a row of
 * k_price_cost is staged in).
 *
 * THE WINDOW RULE.  For a start s and a step offset `step`:   price[k, c] = lib[s + (step + k)*n_chan + c]   for k < len, with len = N_tilde for the cost
 * and 1 for the stage cost.  A start is valid iff s >= 0 and s <= lib_len - (step + len)*n_chan (tested so that nothing overflows).  Every start of every
 * call is tested on the host BEFORE anything is queued, the first offender is named by instance; the largest resident start is remembered on the host, so
 * that a call with start == NULL and another step is tested without reading the device.
 *
 * THE COST OF A RESIDENT BATCH.  mld_set_price_cost: per-model tables owned by the problem like the policy tables -- a_v and sum_v (n_models, n_chan, nv),
 * a_y (n_models, n_chan, ny); any NULL = zeros, all NULL clears.  mld_instance_cost_from_prices, start (batch): builds ON THE DEVICE (k_price_cost) exactly
 * the weights a caller would have uploaded.  With m = model_idx[b] (0 without) and p[k, c] the window of instance b:
 *     S[c]               = p[0,c] + p[1,c] + ... + p[N_tilde-1,c]                                  (k ascending, one rounding per addition)
 *     lin_v[b, k*nv + j] = sum_c ( a_v[m,c,j] * p[k,c] )  +  sum_c ( sum_v[m,c,j] * S[c] )         (c ascending in both sums)
 *     lin_y[b, k*ny + j] = sum_c ( a_y[m,c,j] * p[k,c] )
 * every product and every addition rounded on its own (no fused multiply-add), so the weights are bit-identical to the numpy restatement
 * (pyhybridcontrol_amd/prices.py: cost_np) and the resident cost to the one mld_upload_instance_cost(lin_v, NULL, lin_y) leaves.  a_v on the z column with
 * n_chan = 1 is the reference's q_z = prices_tilde, sum_v on the mu columns its q_mu, a_y a price on an output (exported power).  From there on the call IS
 * mld_upload_instance_cost: the same resident cost with the same row length, the same pull-back GEMM fed from the device-built weights (none, and
 * batch x n doubles, without a_y), the same lifetime -- valid until the next mld_upload_batch, replaced by a later mld_upload_instance_cost and vice
 * versa, kept by mld_select_inputs and the advances, plan and MIP start untouched -- and no consumer sees a difference.  The starts stay resident in an
 * array of their own: start == NULL re-uses them with another step (NULL without resident starts for this batch size is refused).  It moves 8 bytes per
 * instance, or nothing, where the upload moves N_tilde*nv doubles per instance.
 * MLD_ERR_INVALID before anything is queued, nothing changed.  mld_set_price_cost: no price library; a non-finite entry; a_y with ny == 0.
 * mld_instance_cost_from_prices: no batch resident; a launched solve not finished; no price library; no tables; step < 0; an invalid start; a time-varying
 * handle (mld_model_create_tv) -- the ONE restriction against mld_upload_instance_cost, which takes such handles: the tables are per model, not per step model.
 *
 * THE STAGE COST IN THE SIMULATION LOG.  mld_set_stage_cost: per-model weights w_v (n_models, n_chan, nv), w_y (n_models, n_chan, ny); NULL = zeros, all
 * NULL clears (and disarms); needs the price library (no library, a non-finite entry, w_y with ny == 0: refused).  mld_sim_log_cost_begin(start (batch))
 * arms the stage cost for the log that has been begun: cost (capacity, batch) and price (capacity, batch, n_chan) beside the log, filled with NaN, and
 * total (batch), steps (batch), zeros.  From then on every step that writes a log record -- through mld_sim_step_batch, _resolve, _policy or _fallback --
 * also writes into that record's slot (k_stage_cost, one launch behind the step's own kernel)
 *     price[c] = lib[s_b + step*n_chan + c]                              (step: the step call's own argument, the one that slides the realised omega)
 *     cost     = sum_c price[c] * ( sum_j w_v[m,c,j]*v[j] + sum_j w_y[m,c,j]*y[j] )              (c, j ascending; no fused multiply-add)
 * with the record's own v (the slice the plant was stepped with, whatever the entry point applied) and y.  A stepped instance gets total[b] += cost and
 * steps[b] += 1; a skipped one (no usable plan, infeasible auxiliaries) cost = NaN in the record -- price is recorded all the same -- and total and steps
 * stay.  With w_v on the grid model's z this is the reference's sim_k.z * prices_k, and total its total_cost_struct.  The armed state belongs to the log:
 * mld_sim_log_begin and mld_upload_batch discard it, mld_upload_prices disarms.  While armed, a logging step also tests s_max + (step + 1)*n_chan <= lib_len
 * before anything is queued.  Without arming every step entry point queues exactly what it queued before.  Memory: capacity x batch x (1 + n_chan) doubles
 * and batch x (1 double + 1 int + 1 start).
 * MLD_ERR_INVALID, nothing changed: arming without a begun log, without a price library, without stage weights, with start == NULL or an invalid start;
 * mld_download_sim_log_cost -- cost (count, batch), price (count, batch, n_chan), either may be NULL -- with a range outside [0, n_logged] or without an
 * armed log; mld_download_cost_total -- total (batch), steps (batch) -- without an armed log. */
int mld_upload_prices(mld_problem_t *, int64_t lib_len, const double *lib, int n_chan);
int mld_set_price_cost(mld_problem_t *, const double *a_v, const double *sum_v, const double *a_y);
int mld_instance_cost_from_prices(mld_problem_t *, const int64_t *start, int step);
int mld_set_stage_cost(mld_problem_t *, const double *w_v, const double *w_y);
int mld_sim_log_cost_begin(mld_problem_t *, const int64_t *start);
int mld_download_sim_log_cost(mld_problem_t *, int first, int count, double *cost, double *price);
int mld_download_cost_total(mld_problem_t *, double *total, int32_t *steps);

/* ---- campaign KPIs: column statistics of the resident log ----------------------------------------------------------------------------------------------
 * The reference's result of a campaign is grid_sim_dataframe, and every figure its plotting scripts quote is a column statistic of that frame over time
 * (examples/residential_mg_with_pv_and_dewhs/plotting/plot_multi_sim_campaign.py:69-131): cost.sum(axis=0), p_exp.sum(axis=0) with p_exp = y - z
 * (modelling/micro_grid_agents.py:750-753), y.sum(axis=0), mu[..., 0].sum(axis=0), mu[..., 1].sum(axis=0).  mld_sim_log_summary reduces records
 * [first, first + count) of the resident log on the device (k_log_summary) instead of downloading them.
 *
 * KPI q (1 <= n_kpi <= MLD_KPI_MAX) of model m = model_idx[b] is a linear functional of a record, given by up to five per-model tables, each
 * (n_models, n_kpi, width) or NULL: w_x (nx), w_v (nv), w_y (ny), w_omega (nomega), w_xk1 (nx).  A table that was not given adds no term at all.  For the
 * given ones, in the order x, v, y, omega, x_k1:
 *     s_t = sum_i w_t[m,q,i] * field_t[i]          (i ascending, from 0.0)
 *     f   = the sum of the s_t, left to right, beginning with the first given one
 *     f   = price[k,b,c] * f                        where price_chan[q] = c >= 0 (price_chan (n_kpi) or NULL = none priced): the price record of the armed
 *                                                   stage cost (mld_sim_log_cost_begin)
 * every product and every addition rounded on its own (no fused multiply-add), so the results are bit-identical to the numpy restatement
 * (pyhybridcontrol_amd/simlog.py: summary_np).  thresh (n_models, n_kpi) or NULL = +inf.
 * A record k counts for instance b -- is STEPPED -- if and only if x_k1[k,b,0] is not NaN: mld_sim_step_batch's own marking of a skipped instance.
 * Per (b, q), over the stepped records of the range in ascending k -- each output (batch, n_kpi):
 *     sum        sum = sum + f, from 0.0
 *     min, min_step / max, max_step    by strict < / >: the first attaining record wins, a NaN never wins; the steps are absolute record indices;
 *                +inf / -inf / -1 for an instance without a stepped record
 *     n_above    records with f > thresh[m,q]
 *     n_changes  stepped records whose f is != the previous stepped record's f in the range: the switch count of an input channel
 * Per instance -- each output (batch):
 *     n_stepped; vio_max, vio_step of the records' cons_vio by strict > (-inf / -1 when empty); n_vio: stepped records with cons_vio > vio_tol;
 *     nodes_total (int64) over ALL records of the range; n_source (batch, 3): records with u_source == 0 / 1 / 2 (mld_download_sim_log_source), every
 *     entry -1 when the log has no source array.
 * Any output may be NULL.  count == 0 is valid and gives the empty values.  With w_v = mld_set_stage_cost's weights of channel 0, price_chan = 0 and
 * n_chan = 1, sum is mld_download_cost_total's total and n_stepped its steps.
 * The call reads the log and writes nothing on the handle: not the records, the count, the armed totals, the inputs, the plan or the start.  It runs on the
 * problem's stream and waits for it.  Only the fields whose table is given are read (and element 0 of x_k1, cons_vio, nodes, u_source, and the price record
 * where a KPI is priced), each byte once.
 * MLD_ERR_INVALID before anything is queued, the argument named: no batch; a launched solve not finished; no log begun; a range outside [0, n_logged];
 * n_kpi outside 1 .. MLD_KPI_MAX; all five tables NULL; a table of a variable the model has none of (w_y with ny == 0, w_omega with nomega == 0); a
 * non-finite weight; a NaN thresh or vio_tol; price_chan[q] >= 0 without an armed stage cost; price_chan[q] >= n_chan; price_chan[q] < -1; a model without
 * a state (nx == 0: nothing marks the stepped records); a record wider than the kernel's staging (768 doubles). */
#define MLD_KPI_MAX 64      /* the lanes of a wave: one lane owns one KPI */
int mld_sim_log_summary(mld_problem_t *, int first, int count, int n_kpi,
                        const double *w_x, const double *w_v, const double *w_y, const double *w_omega, const double *w_xk1,
                        const int32_t *price_chan, const double *thresh, double vio_tol,
                        double *sum, double *min, double *max, int32_t *min_step, int32_t *max_step, int32_t *n_above, int32_t *n_changes,
                        int32_t *n_stepped, double *vio_max, int32_t *vio_step, int32_t *n_vio, int64_t *nodes_total, int32_t *n_source);

/* ---- rollout KPIs: the same column statistics per rolled-out trajectory -----------------------------------------------------------------------------------
 * mld_rollout_kpi is mld_rollout_batch (policy == 0: u_prev and switches_out are ignored, no resident policy is needed) or mld_rollout_policy (policy != 0)
 * with the KPIs of mld_sim_log_summary reduced inside the rollout kernel (k_rollout_kpi / k_rollout_policy_kpi, two more instantiations of k_rollout's
 * body): what the reference quotes per MPC variant against `thermo` (plot_multi_sim_campaign.py:69-131), for batch x S trajectories of K steps in one
 * launch, without a log, a download of the trajectories or an armed stage cost.  Every argument, ending and output of the two means what it means there and
 * stays available in the same call.
 *
 * The record of trajectory (b, c) at step k in [0, K) is x = x_k, v = v_k = [u; delta; z; mu], y = y_k, omega = the nomega realised values of step k (not
 * the resolver's [omega; u]) and x_k1 = x_{k+1}.  KPI q of model m = model_idx[b] is mld_sim_log_summary's functional of it -- n_kpi, w_x .. w_xk1,
 * price_chan and thresh as there, the same order of operations, no fused multiply-add -- and where price_chan[q] = ch >= 0
 *     f = price * f,   price = lib[price_start[b] + (step + k) * n_chan + ch]
 * of the resident price library (mld_upload_prices): price_start (batch) int64, one tariff for the S realisations of an instance, `step` the rollout's own
 * step, so that step k sees the price mld_sim_step_*(step = step + k) records in a log armed with the same starts.  The price window is the price library's
 * window rule with K steps: 0 <= price_start[b] and price_start[b] + (step + K) * n_chan <= lib_len.
 * Per (b, c, q) over k ascending -- each output (batch, S, n_kpi): sum, min / min_step, max / max_step, n_above, n_changes as mld_sim_log_summary defines
 * them, the steps being k itself (the record indices of a log begun at 0); per (b, c): n_vio (batch, S), the steps with cons_vio > vio_tol.  The figures
 * are bit-identical to those of the logged route -- K advancing mld_sim_step_resolve / mld_sim_step_policy steps of realisation c, then
 * mld_sim_log_summary -- and to simlog.py: rollout_kpis_np on the trajectories.  A trajectory that does not end 0 (infeasible, declined, not attempted)
 * gets NaN in every double and -1 in every integer, the convention of cost_out / mu_total_out / switches_out.  Any output may be NULL.
 * The call is host-synchronous and writes nothing on the handle: inputs, plan, MIP start, log, policy state, resident starts and an armed stage cost stay.
 * MLD_ERR_INVALID before anything is queued, the argument named: everything mld_rollout_batch (and, with policy != 0, mld_rollout_policy) refuses; n_kpi
 * outside 1 .. MLD_KPI_MAX; all five tables NULL; a table of a variable the model has none of; a non-finite weight; a NaN thresh or vio_tol; price_chan[q]
 * outside [-1, n_chan); a priced KPI without a resident price library or with price_start == NULL; a price start whose window leaves the library (the
 * first offender is named); a staging that, with its 6 n_kpi doubles of accumulators, no longer fits a wave's share of LDS. */
int mld_rollout_kpi(mld_problem_t *p, mld_problem_t *aux, int policy, int K, int S, const double *u_seq, const double *u_prev, const double *omega_seq,
                    const int64_t *start, int step, const double *cost_w, int cost_rows, int n_kpi,
                    const double *w_x, const double *w_v, const double *w_y, const double *w_omega, const double *w_xk1,
                    const int32_t *price_chan, const double *thresh, double vio_tol, const int64_t *price_start,
                    double *x_out, double *v_out, double *y_out, double *cons_vio_out, int32_t *cons_row_out,
                    double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out, int32_t *end_status_out,
                    int32_t *switches_out, int64_t stats[4],
                    double *sum, double *min, double *max, int32_t *min_step, int32_t *max_step, int32_t *n_above, int32_t *n_changes, int32_t *n_vio);

/* ---- rollout risk: statistics across a rollout's realisations ------------------------------------------------------------------------------------------------
 * The reference's headline figures are a column statistic over time followed by a reduction over the Monte-Carlo runs, .mean(level=[..., 'controller'])
 * (plot_multi_sim_campaign.py:69-131).  mld_rollout_risk is mld_rollout_kpi (n_kpi >= 1) or mld_rollout_batch / mld_rollout_policy (n_kpi == 0: no KPI table,
 * the KPI arguments are ignored) with that second reduction made on the device, by k_rollout_risk queued behind the rollout kernel on the problem's stream:
 * per instance a few doubles per column instead of every trajectory's.  Every argument, ending and output of the others means what it means there; ANY
 * output may be NULL, the per-trajectory ones included, so a caller that wants only the risk downloads only the risk.
 *
 * A call names G columns (1 <= G <= MLD_RISK_COLS_MAX); column j is (col_src[j], col_q[j]) over the per-trajectory results of the same call:
 *     0 cost   1 mu_total   2 worst_vio   3 switches (policy != 0 only)   4 n_vio   5 / 6 / 7 KPI sum / min / max of KPI col_q[j]
 *     8 / 9 KPI n_above / n_changes of KPI col_q[j]                 (integers become doubles exactly; 4 .. 9 need n_kpi >= 1; col_q is read for 5 .. 9 only)
 * For instance b and column j let g[c] be realisation c's value.  c is COMPLETE iff end_status[b, c] == 0; n is the number of complete realisations.
 *   counts (batch, 4)   over all c: n_complete, n_infeasible (ending 1), n_declined (2), n_not_attempted (-1)
 *   order               the complete c ascending by the pair (g, c): a before a' iff g < g', or g == g' and c < c' -- so -0.0 and +0.0 tie and c decides; a
 *                       NaN sorts after every number, by c: a stable sort by value.  sorted[r], r = 0 .. n - 1.
 *   T(leaf[0 .. 63])    the balanced binary tree over 64 leaves in index order: (0,1), (2,3), ..., then those results pairwise, six levels, every addition
 *                       rounded on its own; a leaf that is not selected is +0.0
 * Per (b, j) -- each output (batch, G):
 *   mean = T(leaf c = g[c] if complete) / n;  min, min_c / max, max_c by strict < / >: the smallest attaining c wins, a NaN never wins;
 *   n_exceed: the complete c with g[c] > level[j] (level (G), or NULL = +inf)
 * Per (b, j, l) for the L levels alpha[l] in (0, 1] (0 <= L <= MLD_RISK_LEVELS_MAX) -- each output (batch, G, L):
 *   i = the smallest i >= 0 with (double)(i + 1) >= alpha[l] * (double)n, the index ceil(alpha n) - 1 (tabulated by the host once per call);
 *   quantile = sorted[i], quantile_c its c;  cvar_hi = T(leaf r = sorted[r], i <= r < n) / (n - i);  cvar_lo = T(leaf r = sorted[r], r <= i) / (i + 1)
 * An instance with n == 0: mean, quantile, cvar_* NaN; min +inf, max -inf; every _c -1; n_exceed 0 (mld_sim_log_summary's conventions).
 * The figures are bit-identical to simlog.py: rollout_risk_np on the per-trajectory outputs of the same call.  The call is host-synchronous and writes nothing
 * on the handle.
 * MLD_ERR_INVALID before anything is queued, the argument named: everything mld_rollout_kpi refuses (n_kpi == 0 aside); S > MLD_RISK_S_MAX; G or L out of
 * range; an unknown source; source 3 with policy == 0; a source >= 4 with n_kpi == 0; col_q[j] outside [0, n_kpi); alpha[l] outside (0, 1] or NaN; a NaN
 * level. */
#define MLD_RISK_COLS_MAX 64
#define MLD_RISK_LEVELS_MAX 8
#define MLD_RISK_S_MAX 64      /* the lanes of a wave: one lane owns one realisation */
int mld_rollout_risk(mld_problem_t *p, mld_problem_t *aux, int policy, int K, int S, const double *u_seq, const double *u_prev, const double *omega_seq,
                     const int64_t *start, int step, const double *cost_w, int cost_rows, int n_kpi,
                     const double *w_x, const double *w_v, const double *w_y, const double *w_omega, const double *w_xk1,
                     const int32_t *price_chan, const double *thresh, double vio_tol, const int64_t *price_start,
                     double *x_out, double *v_out, double *y_out, double *cons_vio_out, int32_t *cons_row_out,
                     double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out, int32_t *end_status_out,
                     int32_t *switches_out, int64_t stats[4],
                     double *sum, double *min, double *max, int32_t *min_step, int32_t *max_step, int32_t *n_above, int32_t *n_changes, int32_t *n_vio,
                     int G, const int32_t *col_src, const int32_t *col_q, const double *level, int L, const double *alpha,
                     double *r_mean, double *r_min, double *r_max, int32_t *r_min_c, int32_t *r_max_c, int32_t *r_n_exceed,
                     double *r_quantile, int32_t *r_quantile_c, double *r_cvar_hi, double *r_cvar_lo, int32_t *counts);

/* ---- plan selection: choose among candidate plans by their rollout risk ----------------------------------------------------------------------------------------
 * A scenario-based controller rolls out several plans -- the one just solved, the shifted previous one, a baseline's nominal sequence, another handle's
 * scenario plan -- under the SAME S realisations and applies the one whose risk is acceptable and whose cost is lowest; the same step is the safety filter
 * in front of mld_sim_step_resolve.  mld_rollout_select is the open loop of mld_rollout_risk over P candidate input sequences per instance in ONE launch
 * (kernels k_rollout_cand / k_rollout_cand_kpi): trajectory (b, p, c) applies candidate p of instance b under realisation c, the disturbance named once
 * for all candidates -- omega_seq (batch, S, K, nomega) or start (batch, S, n_groups) --, x0, the model, the cost_w row, the price start per instance.
 * Candidate 0 is the resident plan's inputs where plan_first != 0 (the plan-state tests of mld_rollout_batch with u_seq == NULL apply; an instance without a
 * usable plan ends -1 for that candidate only); the others are u_cand (batch, P - plan_first, K, nu).  P == 1 with plan_first certifies the plan.
 * Every per-trajectory output is (batch, P, S[, n_kpi]), the risk of candidate (b, p) is mld_rollout_risk's of "instance" b P + p (k_rollout_risk, unchanged):
 * every r_* output is (batch, P, G[, L]), counts (batch, P, 4), stats as before over batch P S trajectories.
 *
 * THE RULE (csrc/plan_select.inc, kernel k_plan_select queued behind k_rollout_risk).  A statistic is (column, kind, level index): kind 0 mean, 1 min,
 * 2 max, 3 n_exceed (as a double), 4 quantile[l], 5 cvar_hi[l], 6 cvar_lo[l] of risk column `column`; the level index is read for 4 .. 6 only.  Candidate
 * (b, p) is ADMISSIBLE iff its count of complete realisations >= min_complete (1 .. S), every one of the n_cons (0 .. MLD_SELECT_CONS_MAX) constraints
 * value(cons_col[k], cons_kind[k], cons_level[k]) <= cons_bound[k] holds (a NaN value fails), and its objective statistic (obj_col, obj_kind, obj_level) is
 * not NaN.  choice[b] is the admissible p whose objective comes first in the order (value, p), strict < on the value: a tie, or -0.0 against +0.0, goes to the
 * smaller p; score[b] its value, n_admissible[b] the count, admissible (batch, P) bytes.  No admissible candidate: choice -1, score NaN.  u_choice
 * (batch, K, nu) is the chosen sequence and u0_choice (batch, nu) its step 0 -- what mld_sim_step_resolve takes as u0 --, NaN where choice is -1.  Every
 * output may be NULL.  The figures are bit-identical to simlog.py: select_plan_np on the per-candidate risk of the same call.  The call is host-synchronous,
 * reads the handle and changes nothing on it.
 * MLD_ERR_INVALID before anything is queued, the argument named: everything mld_rollout_risk refuses for an open-loop call; P outside 1 .. MLD_SELECT_P_MAX;
 * batch x P x S > INT_MAX (tested before S <= MLD_RISK_S_MAX, so a huge S names the trajectories); u_cand NULL where P - plan_first > 0, or not finite; a
 * column, kind or level index out of range (a per-level kind with L == 0 included); a NaN bound; min_complete outside 1 .. S; n_cons outside
 * 0 .. MLD_SELECT_CONS_MAX; cons_col, cons_kind or cons_bound NULL with n_cons > 0.  cons_level may be NULL: level index 0 for every constraint (and so
 * refused where a constraint's kind is per level and L == 0). */
#define MLD_SELECT_P_MAX 64        /* the lanes of a wave: one lane owns one candidate */
#define MLD_SELECT_CONS_MAX 8
int mld_rollout_select(mld_problem_t *p, mld_problem_t *aux, int K, int S, int P, int plan_first, const double *u_cand, const double *omega_seq,
                       const int64_t *start, int step, const double *cost_w, int cost_rows, int n_kpi,
                       const double *w_x, const double *w_v, const double *w_y, const double *w_omega, const double *w_xk1,
                       const int32_t *price_chan, const double *thresh, double vio_tol, const int64_t *price_start,
                       int G, const int32_t *col_src, const int32_t *col_q, const double *level, int L, const double *alpha,
                       int obj_col, int obj_kind, int obj_level, int n_cons, const int32_t *cons_col, const int32_t *cons_kind, const int32_t *cons_level,
                       const double *cons_bound, int min_complete,
                       int32_t *choice, double *score, int32_t *n_admissible, uint8_t *admissible, double *u_choice, double *u0_choice,
                       double *r_mean, double *r_min, double *r_max, int32_t *r_min_c, int32_t *r_max_c, int32_t *r_n_exceed,
                       double *r_quantile, int32_t *r_quantile_c, double *r_cvar_hi, double *r_cvar_lo, int32_t *counts,
                       double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out, int32_t *end_status_out,
                       int64_t stats[4],
                       double *sum, double *min, double *max, int32_t *min_step, int32_t *max_step, int32_t *n_above, int32_t *n_changes, int32_t *n_vio);

/* ---- plan selection with closed-loop rule policies among the candidates --------------------------------------------------------------------------------------
 * The reference quotes every MPC variant against its thermostat, DewhTheromstatController, a FEEDBACK rule u_k = f(x_k, u_{k-1}) stepped in closed loop, and
 * the safety filter's fall-back is that same rule.  A nominal input sequence is not that baseline: under realisation c the rule reacts to the tank that
 * realisation produced.  mld_rollout_select_policy takes mld_rollout_select's arguments and, behind them, T policies in mld_upload_policy's arrays with a
 * leading table axis: pol_sel (T, n_models, nu, nx), pol_on_at, pol_off_at, pol_u_on, pol_u_off, pol_mode (T, n_models, nu).  The candidates of one call, in
 * this order: the resident plan (plan_first: 0 or 1), n_own = P - plan_first - T open-loop sequences u_cand (batch, n_own, K, nu), T policies; P counts all
 * of them, 1 .. MLD_SELECT_P_MAX; trajectory t = (b P + p) S + c, all candidates under the same S realisations.  Kernels k_rollout_cand_policy /
 * k_rollout_cand_policy_kpi: ro_run<true> -- the body of k_rollout_policy -- with a TABLE per candidate: table p - (P - T) for a policy candidate, and for
 * the plan and the sequences one whose every channel is passed through, with which the body copies u_k and counts no switch.  u_prev (batch, nu) is the input
 * before step 0, NULL = the resident policy state as mld_rollout_policy reads it.  switches_out (batch, P, S): the (step, channel) pairs whose input changed,
 * 0 for a complete plan or sequence trajectory, -1 where the trajectory did not end 0; a risk column of source `switches` is accepted in this entry.
 * The choice is k_plan_select's.  The chosen inputs are k_select_inputs' (queued behind it): a plan or sequence pick is copied as before; a policy pick has
 * u0_choice[b, j] = the rule on (x0[b], u_prev[b, j]) -- step 0 of the closed loop, the same bits, what mld_sim_step_resolve takes as u0 --, that row as
 * u_choice[b, 0, :] and NaN in rows 1 .. K - 1, which differ from realisation to realisation; no choice: all NaN.  A policy candidate equals
 * mld_upload_policy followed by mld_rollout_risk(policy = 1) bit for bit, a sequence candidate mld_rollout_risk(u_seq) with switches 0.
 * T == 0 is mld_rollout_select's call: the same kernels, the same bits.  The tables, candidates and choice live in temporaries of the call; the handle is read
 * and never changed -- the resident policy and its state, plan, MIP start, log and starts stay.  Nothing is finished on the host on this entry (as
 * mld_warm_start_from_rollout): a trajectory the LDS solver declines ends 2, is counted in counts[.., 2] and stats[3], and with min_complete == S makes its
 * candidate inadmissible.
 * MLD_ERR_INVALID before anything is queued, the argument named: everything mld_rollout_select refuses; T < 0 or T > P - plan_first; any table entry
 * mld_upload_policy would refuse (the message names table, model and channel); a policy candidate with a passed-through channel (pol_mode == 0) -- a candidate
 * that rules some channels and takes the plan for the others is not built --; a pol_* array NULL with T > 0; u_prev NULL with no resident policy; a
 * non-finite u_prev. */
int mld_rollout_select_policy(mld_problem_t *p, mld_problem_t *aux, int K, int S, int P, int plan_first, const double *u_cand, const double *omega_seq,
                              const int64_t *start, int step, const double *cost_w, int cost_rows, int n_kpi,
                              const double *w_x, const double *w_v, const double *w_y, const double *w_omega, const double *w_xk1,
                              const int32_t *price_chan, const double *thresh, double vio_tol, const int64_t *price_start,
                              int G, const int32_t *col_src, const int32_t *col_q, const double *level, int L, const double *alpha,
                              int obj_col, int obj_kind, int obj_level, int n_cons, const int32_t *cons_col, const int32_t *cons_kind, const int32_t *cons_level,
                              const double *cons_bound, int min_complete,
                              int32_t *choice, double *score, int32_t *n_admissible, uint8_t *admissible, double *u_choice, double *u0_choice,
                              double *r_mean, double *r_min, double *r_max, int32_t *r_min_c, int32_t *r_max_c, int32_t *r_n_exceed,
                              double *r_quantile, int32_t *r_quantile_c, double *r_cvar_hi, double *r_cvar_lo, int32_t *counts,
                              double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out, int32_t *end_status_out,
                              int64_t stats[4],
                              double *sum, double *min, double *max, int32_t *min_step, int32_t *max_step, int32_t *n_above, int32_t *n_changes, int32_t *n_vio,
                              int T, const double *pol_sel, const double *pol_on_at, const double *pol_off_at, const double *pol_u_on, const double *pol_u_off,
                              const int32_t *pol_mode, const double *u_prev, int32_t *switches_out);

/* ---- device completion of declined rollout trajectories -----------------------------------------------------------------------------------------------
 * Every entry of the rollout family -- mld_rollout_batch, _policy, _kpi, _risk, _select, _select_policy, mld_warm_start_from_rollout -- solves the auxiliary
 * problem of a step in LDS, and a trajectory whose step the LDS solver declines ends 2.  mld_set_rollout_completion(p, MLD_ROLLOUT_COMPLETE_DEVICE) makes
 * every later call on the stepped handle p finish those trajectories WITHOUT LEAVING THE DEVICE, after the rollout kernel and before k_rollout_risk,
 * k_plan_select, k_select_inputs or k_warm_from_rollout read anything.  THE RULE is mld_sim_step_resolve's, applied inside a trajectory:
 *   - each declined trajectory t is re-run FROM STEP 0 by the same body, every sum in its order (kernels k_rollout_redo / k_rollout_redo_kpi over the list
 *     k_ro_collect makes of the trajectories with end_status 2);
 *   - at a step the dense solver has already answered, delta, z, mu come from the trajectory's table instead of the LDS solver;
 *   - at the first step k the LDS solver declines without an answer, the wave writes x_k and [omega_k; u_k] -- under a policy the rule's u_k; the bytes
 *     mld_sim_step_resolve(u0 = u_k) would give the resolver at that state -- into a slot of the resolver's input buffers, records k and ends 2 again;
 *   - the listed slots are solved on the resolver's handle by the DENSE kernel, the small path bypassed; k_ro_fix_merge makes the answer table entry (t, k):
 *     usable -- status 0 or 2 with a finite objective and finite values -- or "no feasible point", with which the trajectory ends 1 at step k, NaN / -1 from
 *     there on;
 *   - rounds repeat while a trajectory is still 2.  Each moves every listed trajectory's declining step forward: at most K rounds.
 * The steps before k are re-solved by the same deterministic solver to the same bits, so nothing is kept per trajectory on the common path and the rollout
 * kernels are what they were.  mode 0 (the default): every call queues the launches and returns the results it always did.
 * MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY (tests only, with MLD_ROLLOUT_COMPLETE_DEVICE): MLD_DBG_SMALL_PIVOT_CAP on the resolver then caps the rollout kernel and
 * the first re-run, which finds its declines again, and no later one -- a trajectory with one dense step followed by LDS steps.
 * stats[4] of the entries keeps its meaning: [1], [2] count the FINAL endings, [3] what the rollout kernel declined.  The stepped handle is left as found.
 * On the resolver, the inputs and results of the slots used are put back; a resolver whose resident batch is not the one mld_sim_step_resolve laid out for p's
 * batch is laid out as that call lays it out, by the same test; its work-queue order is forgotten.  A list longer than the slots of its models is solved in chunks.
 * mld_rollout_completion_stats: out = [rounds, finished_on_device, dense_solves, left_declined] of the last call of the family on p (all 0 where nothing
 * was completed).  MLD_ERR_INVALID: p NULL, unknown bits in mode (the mode stays), out NULL. */
#define MLD_ROLLOUT_COMPLETE_DEVICE 1
#define MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY 2
int mld_set_rollout_completion(mld_problem_t *p, int mode);
int mld_rollout_completion_stats(mld_problem_t *p, int64_t out[4]);

/* Per-instance telemetry of the last solve: time spent inside the solve kernel (device wall clock, ns) and
 * the number of dictionary rows the rank-1 updates touched (x *row_bytes x 2 = bytes streamed by pivots). */
int mld_download_telemetry(mld_problem_t *, int64_t *latency_ns, int64_t *rows_updated, int64_t *row_bytes);

/* Constraint right-hand side only (kernel K3): h = H_x x_k + H_w w + H_5 per instance
 * (controllers/controller_base.py:446-450); `scenarios`>1 applies the row-min over scenario columns
 * of H_w Omega (:442-444) with omega laid out (batch, scenarios, N_tilde*nomega).  h_out (batch, N nc).
 * Uses the ORIGINAL (un-tightened) model so that it can populate gen_evo_constraints. */
int mld_rhs_batch(mld_problem_t *, int batch, int scenarios, const int32_t *model_idx, const double *x0,
                  const double *omega, double *h_out);

/* ---- multi-GPU result gather (RCCL over xGMI) ---------------------------------------------
 * One process per GPU.  Rank 0 calls mld_comm_unique_id, the bytes are broadcast by the launcher
 * (any side channel), every rank calls mld_comm_init.  mld_gather all-gathers `count` doubles per
 * rank from a HOST buffer (staged through device memory) into recv (n_ranks*count). */
#define MLD_COMM_ID_BYTES 128
int mld_comm_unique_id(uint8_t id[MLD_COMM_ID_BYTES]);
int mld_comm_init(int n_ranks, int rank, const uint8_t id[MLD_COMM_ID_BYTES]);
int mld_gather(const double *send, int count, double *recv);
/* The result gather of the path straight from the device buffers of the last solve (no host staging of the send side): per
 * instance 2 + nv doubles = (objective, status, step-0 slice [u0; delta0; z0; mu0] -- what `variables_k` hands the caller,
 * controllers/components/variables.py:75-85); every rank contributes its whole batch (equal on all ranks); recv (host) holds
 * n_ranks x batch x (2 + nv), rank-major. */
int mld_gather_results(mld_problem_t *, double *recv, int *width_out);
int mld_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* MLDGPU_H */
