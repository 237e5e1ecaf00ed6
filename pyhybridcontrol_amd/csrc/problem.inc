// solver trace (opts.reserved MLD_DBG_TRACE) is compiled in only with -DMLD_TRACE: device printf in the kernel costs registers
#ifdef MLD_TRACE
#define MLD_PRINTF(...) printf(__VA_ARGS__)
#else
#define MLD_PRINTF(...) ((void)0)
#endif
// Kernels K3 (constraint right-hand side / cost vector per instance), K4 (cost pull-back) and
// K5+K6 (LP relaxation by bounded dual simplex + Gomory mixed-integer cuts + branch-and-bound).
//
// K5/K6 replace the backend call `self._problem.solve(...)` (controllers/controller_base.py:509) that the
// reference hands to cvxpy -> Gurobi.  One workgroup owns one instance at a time and keeps ONE dense
// fp64 dictionary for it in HBM ((m + cuts + 1) x (n + 1) doubles, row-major, rows contiguous):
//   * every simplex pivot is a rank-1 update streamed through the workgroup -- the pivot row and the
//     multiplier column are staged in LDS, each wave owns whole rows and walks them with contiguous
//     512-byte wave accesses; rows whose multiplier is zero are skipped (the dictionary of a cluster
//     of independent tanks stays block-sparse);
//   * branch-and-bound never copies the dictionary: a node is a set of bound changes, every binary is
//     boxed, so ANY basis can be made dual feasible by flipping non-basic variables to the right
//     bound, and the dual simplex re-optimises from wherever the previous node left the basis;
//   * a persistent grid (n_slots workgroups) pulls instances from an atomic counter, so the
//     working set is n_slots dictionaries regardless of the batch size.
// The kernel is bound by HBM traffic on the dictionary (DESIGN.md section 4); MFMA has no role.
#pragma once
#include "common.h"

#ifndef S_RESTART_ROWS
#define S_RESTART_ROWS 0         // cut rows only the root restart may use (0: it takes what the root cut loop left of max_cuts -- 150 rows of its own measured
                                 // -7 % on every pipelined figure of the bench, whether a restart ran or not, for one more proven instance in 256)
#endif
#define S_RESTART_ROUNDS 5        // cut rounds of a root restart
#define S_RESTART_PATIENCE 3      // ... and rounds without progress of the bound before it gives up
#ifndef S_RESTART_GAPS
#define S_RESTART_GAPS 3.0       // the restart runs when the incumbent is within this many gap tolerances of the proven bound (MIPGap 1e-2: 3 %) ...
#endif
#ifndef SOL_NT
#define SOL_NT 512               // threads per workgroup (8 waves)
#endif
#define SOL_NW (SOL_NT / 64)
#ifndef SOL_WPE
#define SOL_WPE 2                // waves per SIMD the kernel is compiled for: 2 = one 512-thread workgroup per CU with 256 VGPRs, 4 = two with 128
#endif
#define S_BIG 1.0e7
#define S_PTOL 1e-8
#define S_PTOL_SKIP 1e-6
#define S_DTOL 1e-9
#define S_PIV_ABS 1e-7
#define S_PIV_REL 1e-7
#define S_PIV_TINY 1e-5
#define S_INTTOL 1e-6
#define S_COEF_ZERO 1e-9
#define S_PURGE_SLACK 1e-3
#define S_RESID_TOL 1e-6
#ifndef S_CUT_PATIENCE
#define S_CUT_PATIENCE 10   // cut rounds without progress of the bound before the cut loop gives up (round 3: was 2 -- on a dual degenerate root the first rounds cut
                            // vertices off the optimal face without moving the bound; stopping there left a steady-state instance at a 3.7 % root gap and 800 nodes
                            // where four more rounds close it in 6 nodes.  oracle ORC_CUT_PATIENCE)
#endif
#define S_MIR_FMIN 0.005          // c-MIR: fractional part of the scaled right-hand side must lie in [S_MIR_FMIN, 1 - S_MIR_FMIN] (round 3: was 0.05; the
                                  // strongest roundings of the tank rows are the "just barely needs one more heating step" ones, f ~ 0.003 .. 0.03)
#define S_PERT 1e-6               // anti-stalling cost perturbation (s_perturb_costs)
#define S_INF (__builtin_huge_val())

enum { LP_OPTIMAL = 0, LP_INFEASIBLE = 1, LP_CUTOFF = 2, LP_ITERLIMIT = 3 };
#define MLD_STATUS_SKIPPED 17    // internal (in-kernel hand-off): an item of a tree that was given up before the item was claimed
#define MLD_STATUS_EXPANDED_OPEN 18   // internal (in-kernel hand-off): the entry gave subtrees away AND left a rest of its own unfinished
#define MLD_STATUS_EXPANDED 16   // internal (in-kernel hand-off): the entry stopped at its node limit and its open nodes were published as items; never returned to the caller

struct SolverShape {
    int n, m0, mcap, ld, ntot, nb, nx, nW, N, nv;
    int first_cap;               // rows (original + cut) the root cut loop may fill; the rows between first_cap and mcap belong to the root restart (S_RESTART_ROWS)
    int max_cuts, cuts_per_round, cut_rounds, max_nodes, max_pivots;
    double gap_abs, gap_rel;
    int debug;
    int presolve;                // 1: per-instance bound propagation before the root LP (s_presolve; mld_opts.presolve bit 2)
    int qp;                      // 1: convex quadratic cost (simplicial decomposition at every node)
    size_t ws_stride;            // bytes per slot
    // offsets (bytes) inside a slot
    size_t oD, oGc, oHc, oLo, oHi, oXB, oXN, oBasic, oNonbasic, oWhere, oAtUp, oSkip, oTmpX, oG, oAx,
        oRootLo, oRootHi, oStkJ, oStkF, oStkS, oSvJ, oSvLo, oSvHi, oKey, oXo,
        oY, oPY, oHm, oCm, oWm, oGcost, oVcur, oPv, oXroot, oFxLo, oFxHi, oFxJ, oMirEff, oMirDelta, oMirCache, oDw, oLive, oMq, oStkV, oClo, oChi;
    int mir_per_round;           // c-MIR cuts per root cut round (0 = off)
    int lMirCache;               // byte offset of the per-wave score lines in LDS, or -1 (they stay in the slot)
    int mir_cap, lMirLine;       // compact c-MIR lines in LDS: 2 * mir_cap doubles per wave (mir_cap >= free binaries of any original row), or lMirLine = -1
    int lDw;                     // devex weights of the rows in LDS, or -1 (they stay in the slot)
    int lCost;                   // reduced-cost row in LDS, or -1 (it stays behind the dictionary in the slot)
    // hot per-basis state kept in LDS when it fits (byte offsets into the dynamic LDS block, -1 = stays in the slot)
    int lLo, lHi, lXB, lXN, lBasic, lNonbasic, lAtUp, lSkip;
    int seccap;                  // entries of the LDS sector list (>= mcap + 8 and >= number of update sectors)
    int lPair;                   // byte offset of the second pivot's staging buffers in LDS (s_bind_slot; they share the bytes of lMirCache, which
                                 // only the cut rounds use), or -1: every pivot updates the dictionary on its own (s_dual_simplex_impl)
    long long time_ticks;        // per-instance budget in wall_clock64 ticks (mld_opts.time_limit; 0 = none): ends the search like max_nodes does
};

// LDS bytes of the second pivot's buffers, in the order s_bind_slot lays them out: the pivot row (n + 2 doubles), the multiplier column (it stages the
// eligible |a| of the look-ahead ratio test first: max(mcap, n) + 2 doubles), the union row and sector lists, one flag byte per update sector
__host__ __device__ inline size_t pair_lds_bytes(int n, int mcap)
{
    const size_t nsec = (size_t)(n + 8) / 8;
    return sizeof(double) * ((size_t)n + 2 + (size_t)(mcap > n ? mcap : n) + 2) + sizeof(unsigned short) * ((size_t)mcap + 8 + nsec + 8) + nsec + 8;
}

struct ProblemDev {               // per-problem read-only device data (per model arrays are n_models x ...)
    const double *Gs;             // m0 x n scaled constraint matrix (tightened model)
    const double *Gp;             // the same with columns in dictionary order (colperm), or null
    const double *rs, *cs;        // row / column scales
    const double *qs;             // n  scaled linear cost
    const double *lb, *ub;        // n  scaled bounds (+-inf allowed)
    const unsigned char *is_int;  // n
    const int *bins;              // nb indices of binaries (same for all models)
    const int *colperm;           // n: variable held by dictionary column c at the start (position-major order)
    const double *Hx, *Hw, *H5;   // tightened condensed maps (m0 x nx, m0 x nW, m0)
    const double *cx, *cw, *c0;   // objective constant: r = c0 + cx.x0 + cw.w
    const double *Ps;             // n_models x n x n scaled Hessian (null = linear cost)
    const double *act_max;        // n_models x m0: largest activity of every row under the MODEL's bounds (+inf when unbounded), or null (s_mark_dead)
    const int *binpos;            // n: position of a structural among the binaries (P.bins), -1 for continuous entries (in-kernel hand-off)
    // the scaled rows Gs once more, sparse: by row (csr_*) and by column (csc_*), nnz_cap entries per model (s_presolve), or null
    const int *csr_ptr, *csc_ptr; const unsigned short *csr_col, *csc_row; const double *csr_val, *csc_val; int nnz_cap;
};

struct BatchDev {
    int batch;
    const int *model_idx;         // may be null
    const double *x0, *omega;     // batch x nx, batch x nW
    unsigned char *fixed;         // batch x nb or null (255 = free); with the in-kernel hand-off cap x nb: the items' fixings are written here
    const unsigned char *warm;    // batch x nb MIP start (values of the binaries; first byte 255 = this instance has none) or null
    double *cutoff;               // batch (cap with the in-kernel hand-off): objective cutoff per instance (value of a known solution, constant term included; +inf = none) or null:
                                  // only points better than it are looked for; INFEASIBLE then means "nothing better exists" (mld_set_cutoffs)
    int *open_depth;              // batch: depth of the search stack when the search ended at a limit inside a COMPLETE search (-1 otherwise), or null
    short *open_var;              // batch x nb: the stack's variables (structural index of the k-th binary: P.bins position), root first
    unsigned char *open_val;      // batch x nb: their current values
    unsigned char *open_flag;     // batch x nb: 1 = both children of that level are accounted for (the sibling needs no node of its own)
    double *hs;                   // batch x m0 scaled rhs (K3 output)
    const double *qs_inst;        // batch x n scaled cost per instance (quadratic atoms make q depend on x0, omega) or null
    const double *rconst;         // batch: extra objective constant (quadratic atoms) or null
    double *v_out, *obj_out, *lb_out;
    int *status_out, *nodes_out, *pivots_out, *cuts_out, *refac_out;
    long long *ticks_out, *rows_out;   // per-instance wall-clock ticks inside the kernel, dictionary rows updated
    long long *prof_out;               // batch x 8 category ticks (may be null)
    int *trace;                        // diagnostics (mld_debug_trace): 16 ints per resident workgroup in HOST memory backed by a file -- instance and stage, readable after a GPU fault; or null
    int *counter;
    const int *order;                  // work-queue position -> instance (longest-first from the previous solve) or null
    // In-kernel sub-tree hand-off (mld_set_handoff; DESIGN section 4d): every per-instance array above has `cap` >= batch entries; entries
    // batch .. cap-1 are ITEMS -- open nodes of searches that stopped at their node limit, published by the workgroup that stopped and solved by
    // whichever workgroup claims them next, as instances of their own (the parent's data, the node's fixings, the parent's incumbent as cutoff).
    int ho;                            // 0 = off
    int cap;                           // entries of the per-instance arrays
    int ho_sub_nodes, ho_max_gen, ho_max_children;
    int *tail;                         // entries reserved so far (starts at batch)
    int *finished;                     // entries completed so far: the launch is over when finished == tail
    int *item_src, *item_root, *item_gen;      // cap: instance whose inputs an entry uses / root instance of its tree / generation (0 = instance)
    long long *item_label;             // cap: position of the node in its tree (root 1, child c of label L: 129 L + c + 1): the deterministic tie-break of the merge
    int *item_ready;                   // cap: 1 once an item's data is complete (release / acquire through system-coherent atomics)
    int *item_children;                // cap: open nodes an entry was split into (0 = not split)
    int ho_donate, ho_rounds;          // a complete search that reaches its node limit hands off its ho_donate shallowest open nodes and goes on, ho_rounds times; then it stops and publishes what is left
    int ho_max_tree;                   // a tree is given up once more than this many items of ONE generation have been published for it ...
    int *tree_count, *tree_dead;       // batch x 9: items published per root and generation so far / batch: the tree has been given up: its items are skipped and the merge keeps the
                                       // root's own result.  (Whether a tree is given up does not depend on the order of the queue: every item's children are
                                       // a function of the item alone, so the count passes the cap in every order or in none.)
};

// ------------------------------------------------------------------------------------------------
// K3: hs[b] = rs .* (H_x x0_b + H_w w_b + H_5)      (controllers/controller_base.py:446-450)
// one workgroup per instance; each wave owns rows, lanes walk the row (coalesced), wave-reduce.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(256) k_rhs(int m0, int nx, int nW, const double *Hx, const double *Hw, const double *H5,
                                            const double *rs, const int *model_idx, const double *x0,
                                            const double *omega, double *hs, int scenarios)
{
    const int b = blockIdx.x, mdl = model_idx ? model_idx[b] : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const double *hx = Hx ? Hx + (size_t)mdl * m0 * nx : nullptr, *hw = Hw ? Hw + (size_t)mdl * m0 * nW : nullptr;
    const double *h5 = H5 + (size_t)mdl * m0;
    const double *xb = x0 + (size_t)b * nx;
    for (int i = wave; i < m0; i += nwv) {
        double s = 0.0;
        if (hx) for (int j = lane; j < nx; j += 64) s += hx[(size_t)i * nx + j] * xb[j];
        s = wave_sum(s);
        double wmin = 0.0;
        if (hw) {
            wmin = S_INF;
            for (int sc = 0; sc < scenarios; ++sc) {       // row-min over scenario columns (controller_base.py:442-444)
                const double *wb = omega + ((size_t)b * scenarios + sc) * nW;
                double t = 0.0;
                for (int j = lane; j < nW; j += 64) t += hw[(size_t)i * nW + j] * wb[j];
                t = wave_sum(t);
                t = __shfl(t, 0, 64);
                wmin = fmin(wmin, t);
            }
        }
        if (lane == 0) hs[(size_t)b * m0 + i] = (s + wmin + h5[i]) * (rs ? rs[(size_t)mdl * m0 + i] : 1.0);
    }
}

// Extra constraint blocks (controller_base.py:411-456 called with other omega columns; set_constraints(other_constraints=...),
// :457-475): every block has the SAME left-hand side H_v (rows are a prefix when its N_tilde is reduced), so stacking
// blocks is a row-wise minimum over right-hand sides:  hs[i] = min(hs[i], rs_i (H_x x0 + H_5 + H_w w_c)_i)  for the rows
// i < col_rows[c] that column c constrains.  One workgroup per instance, a wave per row.
__global__ void __launch_bounds__(256) k_rhs_extra(int m0, int nx, int nW, const double *Hx, const double *Hw, const double *H5,
                                                  const double *rs, const int *model_idx, const double *x0,
                                                  const double *omega_cols, int n_cols, const int *col_rows, double *hs,
                                                  const double *x_cols)      // batch x n_cols x nx: the state each column was generated with, or null = x0
{
    const int b = blockIdx.x, mdl = model_idx ? model_idx[b] : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const double *hx = Hx ? Hx + (size_t)mdl * m0 * nx : nullptr, *hw = Hw ? Hw + (size_t)mdl * m0 * nW : nullptr;
    const double *h5 = H5 + (size_t)mdl * m0;
    const double *xb = x0 + (size_t)b * nx;
    if (!hw) return;                      // without a disturbance map every block equals the standard one
    for (int i = wave; i < m0; i += nwv) {
        double s = 0.0;
        if (hx) for (int j = lane; j < nx; j += 64) s += hx[(size_t)i * nx + j] * xb[j];
        s = wave_sum(s);
        double wmin = S_INF;
        for (int c = 0; c < n_cols; ++c) {
            if (col_rows && i >= col_rows[c]) continue;
            const double *wb = omega_cols + ((size_t)b * n_cols + c) * nW;
            double t = 0.0;
            for (int j = lane; j < nW; j += 64) t += hw[(size_t)i * nW + j] * wb[j];
            if (x_cols && hx) {      // a block generated with an explicit x_k (gen_evo_constraints(x_k=...), controller_base.py:411-416)
                const double *xc = x_cols + ((size_t)b * n_cols + c) * nx;
                for (int j = lane; j < nx; j += 64) t += hx[(size_t)i * nx + j] * (xc[j] - xb[j]);
            }
            t = wave_sum(t);
            t = __shfl(t, 0, 64);
            wmin = fmin(wmin, t);
        }
        if (lane == 0 && wmin < S_INF) {
            const double cand = (s + wmin + h5[i]) * (rs ? rs[(size_t)mdl * m0 + i] : 1.0);
            double *dst = hs + (size_t)b * m0 + i;
            *dst = fmin(*dst, cand);
        }
    }
}

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) double lds_f64;
typedef __attribute__((address_space(3))) double2_t lds_f64x2;
typedef __attribute__((address_space(3))) unsigned short lds_u16;
typedef __attribute__((address_space(3))) unsigned char lds_u8;
typedef __attribute__((address_space(1))) double glb_f64;
typedef __attribute__((address_space(1))) double2_t glb_f64x2;
typedef const __attribute__((address_space(1))) int glb_ci32;
typedef const __attribute__((address_space(1))) unsigned short glb_cu16;
typedef const __attribute__((address_space(1))) double glb_cf64;
// entries a thread-per-row (or per-column) walk over the sparse copy takes together: the column and value loads of a group are issued first, then the loads
// they index, then the group's updates in entry order (one entry per iteration was two dependent round trips per entry)
#ifndef WALK_GROUP
#define WALK_GROUP 8
#endif

// dot products of up to 4 HBM rows with one LDS vector, a wave per row batch: the independent loads are issued before the first use (one dependent
// load per iteration costs a full memory latency each).  All DOT_KC column chunks of the four rows go into registers first (n <= 576: the whole row
// group in one pass, 36 loads in flight; wider rows take several passes), then the multiply-adds run in ascending j per row.  The interleaved load /
// multiply-add loop -- the same sums in the same order, but compiled to a wait before every multiply-add -- stays as the path of MLD_DBG_WALKS_SERIAL.
#ifndef DOT_KC
#define DOT_KC 9
#endif
__device__ __forceinline__ void wave_rows_dot4(const glb_f64 *r0, const glb_f64 *r1, const glb_f64 *r2, const glb_f64 *r3,
                                               const lds_f64 *x, int n, int lane, double out[4], bool serial)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (serial) {
#pragma unroll 4
        for (int j = lane; j < n; j += 64) {
            const double xv = x[j];
            s0 += r0[j] * xv; s1 += r1[j] * xv; s2 += r2[j] * xv; s3 += r3[j] * xv;
        }
    } else {
        for (int j0 = lane; j0 < n; j0 += 64 * DOT_KC) {      // (j0 < n: a lane past the end of the row has no summand, as in the loop above)
            double v0[DOT_KC], v1[DOT_KC], v2[DOT_KC], v3[DOT_KC];
#pragma unroll
            for (int k = 0; k < DOT_KC; ++k) {
                const int j = j0 + k * 64 < n ? j0 + k * 64 : 0;      // (past the end: entry 0 again, loaded without a branch and not used)
                v0[k] = r0[j]; v1[k] = r1[j]; v2[k] = r2[j]; v3[k] = r3[j];
            }
#pragma unroll
            for (int k = 0; k < DOT_KC; ++k) {
                const int j = j0 + k * 64;
                if (j < n) { const double xv = x[j]; s0 += v0[k] * xv; s1 += v1[k] * xv; s2 += v2[k] * xv; s3 += v3[k] * xv; }
            }
        }
    }
    out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3;
}

// ------------------------------------------------------------------------------------------------
// small block-level primitives (SOL_NT threads)
// ------------------------------------------------------------------------------------------------
#define LIST_NCH 8               // row chunks (SOL_NT rows each) whose counts the pivot's list exchange holds: m <= 4096; a larger shape compacts chunk by chunk
struct Shared {
    double r2v[2][SOL_NW];     // single-barrier reductions of the simplex loop: two alternating buffers (see block_max1)
    int r2i[2][SOL_NW];
    int r2j[2][SOL_NW];
    double red_v[SOL_NW];
    double red_w[SOL_NW];
    int red_i[SOL_NW];
    int red_j[SOL_NW];
    // broadcast scalars
    double s_d[8];
    int s_i[8];
    // solver state
    int m;
    int pivots, refactors, since_check;
    int lp_status;
    int perturbed;             // the cost row carries the anti-stalling perturbation (s_dual_simplex_impl)
    int bfrt;                  // long-step ratio test in s_dual_simplex_impl (s_root switches it on for the root LP)
    unsigned long long rows;   // dictionary rows touched by rank-1 updates (traffic accounting)
    int nlive;                 // original rows still maintained (s_mark_dead)
    long long deadline;        // wall_clock64 value at which this instance's time limit ends (0 = none): checked between nodes, between cut rounds and every 128 pivots
    int timed_out;
    int cut_cap;               // rows (original + cut) the cut generators may fill right now: S.first_cap in the root cut loop, S.mcap in the root restart
    // the pivot's own exchange slots: nothing else writes them, so a barrier of the pivot never has to protect them from another primitive's readers
    double piv_el;             // pivot element, written by the thread that stages it (s_pivot_head)
    int lcnt[1 + LIST_NCH][SOL_NW];      // per-wave counts of the sector chunk [0] and of the row chunks [1 ..] of the update lists (list_counts)
#ifdef MLD_PIVOT_PROF
    long long pprof[8];        // ticks: 0 head (stage, scale, x_B, cost row, book-keeping), 1 sector list, 2 row list, 3 update loop of single pivots; 4 .. 7 the same for pairs
    long long pcnt[8];         // 0 single pivots, 1 pairs, 2 long-step ticks, 3 long-step pivots, 4 groups examined, 5 groups passed, 6 pivots with flips
    long long sprof[9];        // ticks of the selection (SEL_CLOCK): 0 loop top, 1 pricing scan and its arg-max, 2 row load, pass 1 and emax, 3 pass 2 and tmax, 4 pass 3 and its
                               // arg-max (plain pivots only); 5 .. 8 the same four parts of the look-ahead (-DMLD_PIVOT_PROF=3: slots 0 .. 4, =4: slots 5 .. 8)
#endif
    long long prof[8];         // ticks: 0 pivot update, 1 simplex selection, 2 cuts, 3 leaf, 4 set_bounds, 5 residual/refactor, 6 setup
#ifdef MLD_CUT_PROF
    long long cprof[15];       // (11..14: phase A of the c-MIR round split -- x gather and fractional list, screen, pass 1 with its wave sums, divisor loop; the
                               // last two on wave 0's clock; -DMLD_CUT_PROF=3 reports them in slots 0..3 of mld_debug_profile) cut separation split: c-MIR scoring (phase A), c-MIR build (phase B), Gomory round; from 3: counts (CUT_COUNT sites) -- cut rounds,
                               // Gomory cuts derived, slack columns substituted in them, c-MIR cuts built, rows substituted in them (nbr), rows scored, their list
                               // entries, (row, divisor) pairs scored
#endif
};
// counts of the diagnostic build -DMLD_CUT_PROF=2 (they replace the clocks in mld_debug_profile, see k_solve): the first lane of a wave adds v to slot k
#ifdef MLD_CUT_PROF
#define CUT_COUNT(sh_, k_, v_) do { if ((threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&(sh_).cprof[k_], (unsigned long long)(v_)); } while (0)
#else
#define CUT_COUNT(sh_, k_, v_) ((void)0)
#endif
// sub-clocks of the selection in the diagnostic build -DMLD_PIVOT_PROF (thread 0's clock, as the pivot's): SEL_CLOCK adds the ticks since t_ to slot k_ and restarts t_
#ifdef MLD_PIVOT_PROF
#define SEL_CLOCK_START(t_) long long t_ = wall_clock64()
#define SEL_CLOCK(sh_, k_, t_) do { const long long now_ = wall_clock64(); if (threadIdx.x == 0) (sh_).sprof[k_] += now_ - (t_); (t_) = now_; } while (0)
#else
#define SEL_CLOCK_START(t_) ((void)0)
#define SEL_CLOCK(sh_, k_, t_) ((void)0)
#endif

__device__ __forceinline__ double block_sum(Shared &sh, double v)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh.red_v[wave] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SOL_NW; ++w) s += sh.red_v[w];
    return s;
}

__device__ __forceinline__ double block_max(Shared &sh, double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh.red_v[wave] = v;
    __syncthreads();
    double s = sh.red_v[0];
#pragma unroll
    for (int w = 1; w < SOL_NW; ++w) s = fmax(s, sh.red_v[w]);
    return s;
}

__device__ __forceinline__ double block_min(Shared &sh, double v) { return -block_max(sh, -v); }

// arg-max with smallest-index tie break; returns index (or -1 if every value is -inf), value in *out
__device__ __forceinline__ int block_argmax(Shared &sh, double v, int idx, double *out)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_down(v, o, 64);
        const int i2 = __shfl_down(idx, o, 64);
        if (v2 > v || (v2 == v && i2 >= 0 && (idx < 0 || i2 < idx))) { v = v2; idx = i2; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { sh.red_v[wave] = v; sh.red_i[wave] = idx; }
    __syncthreads();
    double bv = sh.red_v[0]; int bi = sh.red_i[0];
#pragma unroll
    for (int w = 1; w < SOL_NW; ++w) {
        const double v2 = sh.red_v[w]; const int i2 = sh.red_i[w];
        if (v2 > bv || (v2 == bv && i2 >= 0 && (bi < 0 || i2 < bi))) { bv = v2; bi = i2; }
    }
    *out = bv;
    return bi;
}

// Block reductions with ONE barrier: the waves' partials go to one of two alternating buffers (`par` is a per-thread copy of the
// same sequence on every thread).  A wave can reach the reduction after the next one -- the same buffer again -- only after every wave
// has passed the barrier in between, i.e. has finished reading it.  Used in the dual simplex loop (four reductions per pivot).
__device__ __forceinline__ double block_max1(Shared &sh, double v, int &par)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    par ^= 1;
    if ((threadIdx.x & 63) == 0) sh.r2v[par][threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh.r2v[par][0];
#pragma unroll
    for (int w = 1; w < SOL_NW; ++w) s = fmax(s, sh.r2v[par][w]);
    return s;
}
__device__ __forceinline__ double block_min1(Shared &sh, double v, int &par) { return -block_max1(sh, -v, par); }
__device__ __forceinline__ int block_argmax1(Shared &sh, double v, int idx, double *out, int &par)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_down(v, o, 64);
        const int i2 = __shfl_down(idx, o, 64);
        if (v2 > v || (v2 == v && i2 >= 0 && (idx < 0 || i2 < idx))) { v = v2; idx = i2; }
    }
    par ^= 1;
    if ((threadIdx.x & 63) == 0) { sh.r2v[par][threadIdx.x >> 6] = v; sh.r2i[par][threadIdx.x >> 6] = idx; }
    __syncthreads();
    double bv = sh.r2v[par][0]; int bi = sh.r2i[par][0];
#pragma unroll
    for (int w = 1; w < SOL_NW; ++w) {
        const double v2 = sh.r2v[par][w]; const int i2 = sh.r2i[par][w];
        if (v2 > bv || (v2 == bv && i2 >= 0 && (bi < 0 || i2 < bi))) { bv = v2; bi = i2; }
    }
    *out = bv;
    return bi;
}

// The same three reductions without the LDS crossbar and without a branch (the selection of s_dual_simplex_impl and s_look_ahead; MLD_DBG_SELECT_R6 keeps the
// primitives above).  A wave's maximum is six DPP steps on the two halves of the double -- the lane pairs and quad halves of a quad (quad_perm), the two
// quads of eight lanes (row_half_mirror), the two halves of a row (row_mirror): every lane of a 16-lane row then holds the row's maximum; row_bcast:15 into
// rows 1 and 3 and row_bcast:31 into rows 2 and 3 leave the wave's maximum in row 3 -- read from lane 63 into scalar registers.  max and min are exact, so
// the order of the steps does not matter to the bits as long as no operand is NaN and +0.0 / -0.0 do not meet (every caller: see its comment).
template <int CTRL, int ROWS> __device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xf, false); }      // (a row outside ROWS keeps its own value)
template <int CTRL, int ROWS> __device__ __forceinline__ double dpp_f64(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = dpp_i32<CTRL, ROWS>((int)b), hi = dpp_i32<CTRL, ROWS>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned int)lo);
}
#define DPP_XOR1 0xB1            // quad_perm:[1,0,3,2]
#define DPP_XOR2 0x4E            // quad_perm:[2,3,0,1]
#define DPP_HALF_MIRROR 0x141
#define DPP_MIRROR 0x140
#define DPP_BCAST15 0x142
#define DPP_BCAST31 0x143
__device__ __forceinline__ double wave_max_dpp(double v)      // the same value on every lane (it is uniform: scalar registers)
{
    v = fmax(v, dpp_f64<DPP_XOR1, 0xf>(v));
    v = fmax(v, dpp_f64<DPP_XOR2, 0xf>(v));
    v = fmax(v, dpp_f64<DPP_HALF_MIRROR, 0xf>(v));
    v = fmax(v, dpp_f64<DPP_MIRROR, 0xf>(v));
    v = fmax(v, dpp_f64<DPP_BCAST15, 0xa>(v));
    v = fmax(v, dpp_f64<DPP_BCAST31, 0xc>(v));
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned int)lo);
}
__device__ __forceinline__ int wave_min_i32_dpp(int v)
{
    v = min(v, dpp_i32<DPP_XOR1, 0xf>(v));
    v = min(v, dpp_i32<DPP_XOR2, 0xf>(v));
    v = min(v, dpp_i32<DPP_HALF_MIRROR, 0xf>(v));
    v = min(v, dpp_i32<DPP_MIRROR, 0xf>(v));
    v = min(v, dpp_i32<DPP_BCAST15, 0xa>(v));
    v = min(v, dpp_i32<DPP_BCAST31, 0xc>(v));
    return __builtin_amdgcn_readlane(v, 63);
}
// One barrier and the alternating buffers of block_max1; the eight partials are read together and combined in registers.
__device__ __forceinline__ double block_max1_dpp(Shared &sh, double v, int &par)
{
    const double m = wave_max_dpp(v);
    par ^= 1;
    if ((threadIdx.x & 63) == 0) sh.r2v[par][threadIdx.x >> 6] = m;
    __syncthreads();
    double p[SOL_NW];
#pragma unroll
    for (int w = 0; w < SOL_NW; ++w) p[w] = sh.r2v[par][w];
#pragma unroll
    for (int s = SOL_NW / 2; s > 0; s >>= 1)
#pragma unroll
        for (int w = 0; w < s; ++w) p[w] = fmax(p[w], p[w + s]);
    return p[0];
}
__device__ __forceinline__ double block_min1_dpp(Shared &sh, double v, int &par) { return -block_max1_dpp(sh, -v, par); }
// block_argmax1's rule -- the largest value; among equal values the smallest index >= 0; -1 when no lane with the largest value has an index -- in two
// reductions: the maximum of the values, then the minimum over the indices >= 0 of the lanes that hold it (0x7fffffff: none).  block_argmax1's comparison is
// a total order on (value, has an index, -index), so it returns the largest element under that order whatever the order of its steps, and this is that
// element, provided no value is NaN.  (+0.0 and -0.0 compare equal in both: only *out could differ in its sign; no caller passes a zero.)
__device__ __forceinline__ int block_argmax1_dpp(Shared &sh, double v, int idx, double *out, int &par)
{
    const double m = wave_max_dpp(v);
    const int k = wave_min_i32_dpp((v == m && idx >= 0) ? idx : 0x7fffffff);
    par ^= 1;
    if ((threadIdx.x & 63) == 0) { sh.r2v[par][threadIdx.x >> 6] = m; sh.r2i[par][threadIdx.x >> 6] = k; }
    __syncthreads();
    double p[SOL_NW], q[SOL_NW]; int ki[SOL_NW];
#pragma unroll
    for (int w = 0; w < SOL_NW; ++w) { p[w] = q[w] = sh.r2v[par][w]; ki[w] = sh.r2i[par][w]; }
#pragma unroll
    for (int s = SOL_NW / 2; s > 0; s >>= 1)
#pragma unroll
        for (int w = 0; w < s; ++w) q[w] = fmax(q[w], q[w + s]);
    const double bv = q[0];
#pragma unroll
    for (int w = 0; w < SOL_NW; ++w) ki[w] = p[w] == bv ? ki[w] : 0x7fffffff;
#pragma unroll
    for (int s = SOL_NW / 2; s > 0; s >>= 1)
#pragma unroll
        for (int w = 0; w < s; ++w) ki[w] = min(ki[w], ki[w + s]);
    *out = bv;
    return ki[0] == 0x7fffffff ? -1 : ki[0];
}
// the primitive the selection uses (r6: MLD_DBG_SELECT_R6, a constant of the instantiation)
__device__ __forceinline__ double sel_max1(Shared &sh, double v, int &par, bool r6) { return r6 ? block_max1(sh, v, par) : block_max1_dpp(sh, v, par); }
__device__ __forceinline__ double sel_min1(Shared &sh, double v, int &par, bool r6) { return r6 ? block_min1(sh, v, par) : block_min1_dpp(sh, v, par); }
__device__ __forceinline__ int sel_argmax1(Shared &sh, double v, int idx, double *out, int &par, bool r6)
{
    return r6 ? block_argmax1(sh, v, idx, out, par) : block_argmax1_dpp(sh, v, idx, out, par);
}

// arg-min over integer keys (smallest key wins); returns payload of the winner or -1
__device__ __forceinline__ int block_argmin_int(Shared &sh, int key, int payload)
{
    for (int o = 32; o > 0; o >>= 1) {
        const int k2 = __shfl_down(key, o, 64), p2 = __shfl_down(payload, o, 64);
        if (k2 < key) { key = k2; payload = p2; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { sh.red_i[wave] = key; sh.red_j[wave] = payload; }
    __syncthreads();
    int bk = sh.red_i[0], bp = sh.red_j[0];
#pragma unroll
    for (int w = 1; w < SOL_NW; ++w) if (sh.red_i[w] < bk) { bk = sh.red_i[w]; bp = sh.red_j[w]; }
    return bk == 0x7fffffff ? -1 : bp;
}

// ordered (deterministic) compaction of one SOL_NT-wide chunk: thread with `flag` appends `value` at list[base + rank]
// where rank = number of flagged threads with a smaller thread index; returns the new length (same on all threads)
__device__ __forceinline__ int block_compact(Shared &sh, bool flag, unsigned short value, unsigned short *list, int base)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    __syncthreads();
    if (lane == 0) sh.red_i[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < SOL_NW; ++q) { const int cq = sh.red_i[q]; if (q < wave) off += cq; tot += cq; }
    if (flag) list[base + off + __popcll(bal & ((1ull << lane) - 1ull))] = value;
    return base + tot;
}

// The update lists of a pivot in ONE exchange (s_pivot_update, s_pivot_pair) instead of two barriers per SOL_NT-wide chunk: every wave writes the counts of
// its ballots for ALL chunks to its own slots sh.lcnt[chunk][wave], one barrier follows, and every thread sums the slots of a chunk -- the waves before its own
// (its offset) and all of them (the chunk's total) -- and scatters; the lists come out in the order of block_compact, chunk by chunk.  A slot carries up to
// three counts of 10 bits (LIST_PACK: flag 1, flag 2, both; a chunk has at most SOL_NT = 512 members, so the sums of a chunk stay inside their fields).
// sh.lcnt has no other user and two barriers separate its readers from the next pivot's writers (the one before the update and the one after it).
#define LIST_PACK(b1_, b2_) (__popcll(b1_) | (__popcll(b2_) << 10) | (__popcll((b1_) & (b2_)) << 20))
#define LIST_UNION(x_) (((x_) & 1023) + (((x_) >> 10) & 1023) - ((x_) >> 20))      // members with flag 1 or flag 2
__device__ __forceinline__ void list_counts(const Shared &sh, int chunk, int wave, int &off, int &tot)
{
    off = 0; tot = 0;
#pragma unroll
    for (int q = 0; q < SOL_NW; ++q) { const int cq = sh.lcnt[chunk][q]; if (q < wave) off += cq; tot += cq; }
}

// ------------------------------------------------------------------------------------------------
// per-slot workspace view
// ------------------------------------------------------------------------------------------------
struct Ws {
    double *D, *Gc, *hc, *lo, *hi, *xB, *xN, *tmpx, *g, *ax, *root_lo, *root_hi, *sv_lo, *sv_hi, *key, *xo, *dw;
    unsigned short *live;       // original rows that can bind (s_mark_dead), ascending; sh.nlive of them
    int *basic, *nonbasic, *where, *stk_j, *sv_j;
    unsigned char *at_upper, *skip, *stk_first, *stk_second, *stk_val;
    // per-instance read-only
    const double *Gs, *hs, *qs, *cs;
    const double *Gp;        // Gs in dictionary column order (null: gather through colperm)
    const unsigned char *is_int;
    const int *bins, *colperm;
    int n, m0, mcap, ld, nb, dbg;
    int nc_step, nv_step;    // constraint rows / decision variables per horizon step (0 = unknown)
    double *rowr, *colc;   // LDS staging: n+1 and mcap doubles
    unsigned short *seclist; // LDS: active 64-byte sectors of the pivot row
    unsigned short *rowlist; // LDS: rows with a non-zero multiplier
    double *dabuf;           // LDS: n doubles (ratio-test staging)
    // second pivot of a fused pair (SolverShape::lPair; null / 0 when the shape has no room): its row and multiplier column, the union lists of the
    // fused update and, per update sector, bit 0 = active in the first pivot's row, bit 1 = in the second's
    double *rowr2, *colc2; unsigned short *rowlist2, *seclist2; unsigned char *secflag; int pair;
    const double *P;         // scaled Hessian of this instance's model (null = LP)
    double *Y, *PY, *Hm, *cm, *wm, *gcost, *vcur, *Pv, *mq;
    double *mir_eff, *mir_delta;     // m0: best c-MIR efficacy / divisor per original row
    double *mir_cache;               // SOL_NW x 2n: per-wave compact lists (complemented coefficient, complemented value) of the row's free binaries
    int mir_in_lds;                  // the lines live in LDS (typed ds_* accesses)
    int *trace;                      // diagnostics: this workgroup's 16 ints of BatchDev::trace (host memory), or null
    int dc_lds;                      // dcost points into LDS
    int all_lds;                     // every hot array of the pivot loop (xB, xN, lo, hi, dw, dcost, basic, nonbasic, at_upper, skip) is in LDS: typed instantiation (HotT<true>)
    double *dcost;                   // reduced-cost row d[0..n] (d[n] = objective constant): LDS when it fits, else D + mcap * ld
    double *mir_line; int mir_cap;   // compact per-wave lines of the c-MIR scoring in LDS (SOL_NW x 2 mir_cap), or null
    double *xroot, *fx_lo, *fx_hi;   // nb: root relaxation values of the binaries; saved root bounds of RINS fixings
    const int *csr_ptr; const unsigned short *csr_col; const double *csr_val;      // this instance's model: sparse copy of the scaled original rows (s_presolve), or null
    const int *csc_ptr; const unsigned short *csc_row;      // the same by columns (row indices only: the screen of s_mir_round), or null
    double *clo, *chi;               // n: bounds the c-MIR builder and the dead-row test use for the structurals (s_presolve: implied bounds of this instance; the LP's own otherwise)
    int *fx_j;
};

// Binds the workspace of one slot (this workgroup's part of the solver's workspace, ws_base + blockIdx.x * S.ws_stride) and the LDS: the hot arrays
// the shape placed in LDS (S.l* >= 0) live there, the rest in the slot
__device__ __forceinline__ void s_bind_slot(Ws &w, const SolverShape &S, unsigned char *base, double *lds)
{
    w.D = (double *)(base + S.oD); w.Gc = (double *)(base + S.oGc); w.hc = (double *)(base + S.oHc);
    w.lo = (double *)(base + S.oLo); w.hi = (double *)(base + S.oHi); w.xB = (double *)(base + S.oXB);
    w.xN = (double *)(base + S.oXN); w.basic = (int *)(base + S.oBasic); w.nonbasic = (int *)(base + S.oNonbasic);
    w.where = (int *)(base + S.oWhere); w.at_upper = base + S.oAtUp; w.skip = base + S.oSkip;
    w.tmpx = (double *)(base + S.oTmpX); w.g = (double *)(base + S.oG); w.ax = (double *)(base + S.oAx);
    w.root_lo = (double *)(base + S.oRootLo); w.root_hi = (double *)(base + S.oRootHi);
    w.stk_j = (int *)(base + S.oStkJ); w.stk_first = base + S.oStkF; w.stk_second = base + S.oStkS;
    w.sv_j = (int *)(base + S.oSvJ); w.sv_lo = (double *)(base + S.oSvLo); w.sv_hi = (double *)(base + S.oSvHi);
    w.key = (double *)(base + S.oKey); w.xo = (double *)(base + S.oXo);
    w.dw = (double *)(base + S.oDw); w.live = (unsigned short *)(base + S.oLive); w.mq = (double *)(base + S.oMq); w.stk_val = base + S.oStkV;
    w.Y = (double *)(base + S.oY); w.PY = (double *)(base + S.oPY); w.Hm = (double *)(base + S.oHm); w.cm = (double *)(base + S.oCm);
    w.wm = (double *)(base + S.oWm); w.gcost = (double *)(base + S.oGcost); w.vcur = (double *)(base + S.oVcur); w.Pv = (double *)(base + S.oPv);
    w.mir_eff = (double *)(base + S.oMirEff); w.mir_delta = (double *)(base + S.oMirDelta); w.mir_cache = (double *)(base + S.oMirCache);
    w.clo = (double *)(base + S.oClo); w.chi = (double *)(base + S.oChi);
    w.xroot = (double *)(base + S.oXroot); w.fx_lo = (double *)(base + S.oFxLo); w.fx_hi = (double *)(base + S.oFxHi); w.fx_j = (int *)(base + S.oFxJ);
    w.n = S.n; w.m0 = S.m0; w.mcap = S.mcap; w.ld = S.ld; w.nb = S.nb; w.dbg = S.debug;
    w.nv_step = S.nv; w.nc_step = (S.N > 0 && S.m0 % S.N == 0) ? S.m0 / S.N : 0;
    w.rowr = lds; w.colc = lds + (S.n + 2); w.dabuf = lds + (S.n + 2) + (S.mcap + 2);
    w.seclist = (unsigned short *)(lds + (S.n + 2) + (S.mcap + 2) + (S.n + 2));
    w.rowlist = w.seclist + S.seccap;
    unsigned char *lb8 = (unsigned char *)lds;
    w.pair = S.lPair >= 0 && !(S.debug & MLD_DBG_NO_PIVOT_PAIRS);
    w.rowr2 = w.colc2 = nullptr; w.rowlist2 = w.seclist2 = nullptr; w.secflag = nullptr;
    if (S.lPair >= 0) {      // (pair_lds_bytes)
        w.rowr2 = (double *)(lb8 + S.lPair); w.colc2 = w.rowr2 + (S.n + 2);
        w.rowlist2 = (unsigned short *)(w.colc2 + ((S.mcap > S.n ? S.mcap : S.n) + 2)); w.seclist2 = w.rowlist2 + (S.mcap + 8);
        w.secflag = (unsigned char *)(w.seclist2 + ((S.n + 8) / 8 + 8));
    }
    if (S.lXB >= 0) w.xB = (double *)(lb8 + S.lXB); if (S.lXN >= 0) w.xN = (double *)(lb8 + S.lXN); if (S.lLo >= 0) w.lo = (double *)(lb8 + S.lLo);
    if (S.lHi >= 0) w.hi = (double *)(lb8 + S.lHi); if (S.lBasic >= 0) w.basic = (int *)(lb8 + S.lBasic); if (S.lNonbasic >= 0) w.nonbasic = (int *)(lb8 + S.lNonbasic);
    if (S.lAtUp >= 0) w.at_upper = lb8 + S.lAtUp; if (S.lSkip >= 0) w.skip = lb8 + S.lSkip; if (S.lDw >= 0) w.dw = (double *)(lb8 + S.lDw);
    w.dcost = S.lCost >= 0 ? (double *)(lb8 + S.lCost) : w.D + (size_t)w.mcap * w.ld; w.dc_lds = S.lCost >= 0;
    w.all_lds = S.lXB >= 0 && S.lXN >= 0 && S.lLo >= 0 && S.lHi >= 0 && S.lBasic >= 0 && S.lNonbasic >= 0 && S.lAtUp >= 0 && S.lSkip >= 0 && S.lDw >= 0 && S.lCost >= 0;
    w.mir_in_lds = S.lMirCache >= 0;
    w.mir_line = S.lMirLine >= 0 ? (double *)(lb8 + S.lMirLine) : nullptr; w.mir_cap = S.mir_cap;
    if (S.lMirCache >= 0) w.mir_cache = (double *)(lb8 + S.lMirCache);
}

// Typed views of the hot per-basis state for the pivot loop (round 4): when EVERY hot array lives in LDS (Ws::all_lds: the bench shapes) the dual simplex and
// the rank-1 update are instantiated with address_space(3) pointers -- ds_* instructions on one counter -- instead of the generic pointers of Ws, whose
// flat_* accesses wait on the vector-memory AND the LDS counter (227 of them in the loop before).  The other instantiation keeps the generic pointers.
template <bool L> struct HotT;
template <> struct HotT<true> {
    typedef __attribute__((address_space(3))) double *f64p; typedef __attribute__((address_space(3))) int *i32p; typedef __attribute__((address_space(3))) unsigned char *u8p;
};
template <> struct HotT<false> { typedef double *f64p; typedef int *i32p; typedef unsigned char *u8p; };
// the same for what the cut rounds read besides: read-only instance data in global memory and the workgroup's lists in LDS
template <bool L> struct CutT;
template <> struct CutT<true> {
    typedef const __attribute__((address_space(1))) unsigned char *cu8p; typedef const __attribute__((address_space(1))) double *cf64p;
    typedef __attribute__((address_space(1))) double *gf64p; typedef __attribute__((address_space(3))) unsigned short *u16p;
};
template <> struct CutT<false> { typedef const unsigned char *cu8p; typedef const double *cf64p; typedef double *gf64p; typedef unsigned short *u16p; };
#define HOT_VIEW(L_, w_) \
    typename HotT<L_>::f64p h_xB = (typename HotT<L_>::f64p)(w_).xB, h_xN = (typename HotT<L_>::f64p)(w_).xN, h_lo = (typename HotT<L_>::f64p)(w_).lo, h_hi = (typename HotT<L_>::f64p)(w_).hi, \
                            h_dw = (typename HotT<L_>::f64p)(w_).dw, h_d = (typename HotT<L_>::f64p)(w_).dcost; \
    typename HotT<L_>::i32p h_basic = (typename HotT<L_>::i32p)(w_).basic, h_nonbasic = (typename HotT<L_>::i32p)(w_).nonbasic; \
    typename HotT<L_>::u8p h_up = (typename HotT<L_>::u8p)(w_).at_upper, h_skip = (typename HotT<L_>::u8p)(w_).skip

__device__ __forceinline__ const double *orig_row(const Ws &w, int i) { return i < w.m0 ? w.Gs + (size_t)i * w.n : w.Gc + (size_t)(i - w.m0) * w.n; }
__device__ __forceinline__ double orig_rhs(const Ws &w, int i) { return i < w.m0 ? w.hs[i] : w.hc[i - w.m0]; }

// Index assertions of the diagnostic build (-DMLD_ASSERT; compiled out otherwise): every index that is read from a list or an index array is checked
// before it addresses memory; the FIRST failure of a workgroup goes to its slots 4..9 of the mld_debug_trace buffer (code, two values, count - 1 in
// slot 7, instance, stage) -- host memory backed by a file, so the record survives a fault that takes the process down.  Codes: see MLD_CHECK sites.
#ifdef MLD_ASSERT
__device__ __noinline__ void mld_assert_fail(int *trace, int code, long long a, long long b)
{
    if (!trace) return;
    const int k = atomicAdd(&trace[7], 1);          // (slots start at -1: memset 0xff)
    if (k == -1) { trace[4] = code; trace[5] = (int)a; trace[6] = (int)b; trace[8] = trace[0]; trace[9] = trace[1]; __threadfence_system(); }
}
#define MLD_CHECK(w_, cond_, code_, a_, b_) do { if (!(cond_)) mld_assert_fail((w_).trace, (code_), (long long)(a_), (long long)(b_)); } while (0)
#else
#define MLD_CHECK(w_, cond_, code_, a_, b_) ((void)0)
#endif

// Per-instance presolve (round 4; mld_opts.presolve bit 2; oracle/mld_oracle.c presolve_instance runs the same passes): row-activity bound propagation with
// integer rounding (Savelsbergh 1994, section 3.2) on the scaled rows of THIS instance.  The right-hand side carries the instance's x0 and omega, so bounds
// follow that no per-model tightening can know: the grid power of step k lies between omega_k and omega_k + sum P_i, so z_k -- free in the model -- gets
// finite bounds and a step whose omega_k decides the sign has its delta_k fixed.  Jacobi passes over the sparse copies of the rows: a thread per row adds up
// the smallest activity under the bounds of the pass before, then a thread per column takes the tightest bound its rows imply; no atomics, the result does
// not depend on the order of anything.  What is done with the implied bounds:
//   * binaries the propagation fixes are fixed in the LP (w.lo / w.hi);
//   * the implied bounds of the CONTINUOUS structurals go to w.clo / w.chi only.  The LP keeps its own bounds -- a free z stays free and basic; making the
//     implied bounds LP bounds doubles the dictionary's fill (measured on the CPU restatement: +38 % row updates) -- but the c-MIR builder substitutes them
//     (a row with a free continuous entry was unusable before: on the steady-state closed-loop instances the root gap that remains after the cut loop
//     shrinks by half and the hard tail goes from 5 to 1 unproven of 256) and s_mark_dead adds them up (198 instead of ~60 of the 500 rows of a cfg4
//     instance can never bind and are not maintained: the root LP's row updates fall 4 x).
// Row statistics live in the c-MIR score arrays (idle here).  Returns false when the rows are infeasible under the bounds.  All threads call.
#define S_PRE_PASSES 8
__device__ __noinline__ bool s_presolve(const Ws &w, Shared &sh, const ProblemDev &P, int mdl)
{
    const int tid = threadIdx.x, n = w.n, m0 = w.m0;
    const int *rp = P.csr_ptr + (size_t)mdl * (m0 + 1), *cp = P.csc_ptr + (size_t)mdl * (n + 1);
    const unsigned short *rc = P.csr_col + (size_t)mdl * P.nnz_cap, *cr = P.csc_row + (size_t)mdl * P.nnz_cap;
    const double *rv = P.csr_val + (size_t)mdl * P.nnz_cap, *cv = P.csc_val + (size_t)mdl * P.nnz_cap;
    double *rtot = w.mir_eff; int *rmeta = (int *)w.mir_delta;      // -1: every term finite, >= 0: the one column with an infinite term, -2: more than one / no such row
    // typed views of the same arrays for the grouped walks (all in global memory: the model's sparse copies, the instance's right-hand side, this slot)
    glb_cu16 *grc = (glb_cu16 *)rc, *gcr = (glb_cu16 *)cr; glb_cf64 *grv = (glb_cf64 *)rv, *gcv = (glb_cf64 *)cv;
    glb_cf64 *glo = (glb_cf64 *)w.clo, *ghi = (glb_cf64 *)w.chi, *gtot = (glb_cf64 *)rtot, *ghs = (glb_cf64 *)w.hs; glb_ci32 *gmeta = (glb_ci32 *)rmeta;
    const bool serial = (w.dbg & MLD_DBG_WALKS_SERIAL) != 0;
    bool ok = true;
    __syncthreads();
    for (int pass = 0; pass < S_PRE_PASSES; ++pass) {
        double flag = 0.0;
        for (int i = tid; i < m0; i += SOL_NT) {
            const double h = w.hs[i];
            if (h >= 1.0e29) { rmeta[i] = -2; continue; }
            double sum = 0.0; int ninf = 0, jinf = -1;
            const int e1 = rp[i + 1];
            MLD_CHECK(w, rp[i] >= 0 && e1 <= P.nnz_cap && rp[i] <= e1, 140, rp[i], e1);
            if (serial)
            for (int e = rp[i]; e < e1; ++e) {
                const int j = rc[e]; const double g = rv[e];
                MLD_CHECK(w, j < n, 141, j, n);
                const double b = g > 0.0 ? w.clo[j] : w.chi[j];
                if (fabs(b) >= 0.5 * S_BIG) { ninf++; jinf = j; } else sum += g * b;
            }
            else
            for (int e = rp[i]; e < e1; e += WALK_GROUP) {
                int cj[WALK_GROUP]; double cg[WALK_GROUP], cb[WALK_GROUP];
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) { const int eq = min(e + q, e1 - 1); cj[q] = grc[eq]; cg[q] = grv[eq]; MLD_CHECK(w, cj[q] < n, 141, cj[q], n); }
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) cb[q] = cg[q] > 0.0 ? glo[cj[q]] : ghi[cj[q]];
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) if (e + q < e1) { if (fabs(cb[q]) >= 0.5 * S_BIG) { ninf++; jinf = cj[q]; } else sum += cg[q] * cb[q]; }
            }
            rtot[i] = sum; rmeta[i] = ninf == 0 ? -1 : (ninf == 1 ? jinf : -2);
            if (ninf == 0 && sum > h + 1e-6 * fmax(1.0, fabs(h))) flag = 2.0;
        }
        if (block_max(sh, flag) > 1.0) { ok = false; break; }
        flag = 0.0;
        for (int j = tid; j < n; j += SOL_NT) {
            double lo = w.clo[j], hi = w.chi[j];
            const double lo0 = lo, hi0 = hi;
            const bool isint = w.is_int[j] != 0;
            const int e1 = cp[j + 1];
            if (serial)
            for (int e = cp[j]; e < e1; ++e) {
                const int i = cr[e]; const double g = cv[e];
                MLD_CHECK(w, i < m0, 142, i, m0);
                const int mt = rmeta[i];
                if (mt == -2 || (mt >= 0 && mt != j)) continue;
                const double rest = mt == j ? rtot[i] : rtot[i] - g * (g > 0.0 ? lo0 : hi0);
                double b = (w.hs[i] - rest) / g;
                if (g > 0.0) {
                    if (isint) b = floor(b + 1e-6);
                    if (b < hi - 1e-9 * fmax(1.0, fabs(b))) hi = b;
                } else {
                    if (isint) b = ceil(b - 1e-6);
                    if (b > lo + 1e-9 * fmax(1.0, fabs(b))) lo = b;
                }
            }
            else
            for (int e = cp[j]; e < e1; e += WALK_GROUP) {
                int ci[WALK_GROUP], cm[WALK_GROUP]; double cg[WALK_GROUP], ct[WALK_GROUP], ch[WALK_GROUP];
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) { const int eq = min(e + q, e1 - 1); ci[q] = gcr[eq]; cg[q] = gcv[eq]; MLD_CHECK(w, ci[q] < m0, 142, ci[q], m0); }
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) { cm[q] = gmeta[ci[q]]; ct[q] = gtot[ci[q]]; ch[q] = ghs[ci[q]]; }
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) {
                    if (e + q >= e1) continue;
                    const double g = cg[q]; const int mt = cm[q];
                    if (mt == -2 || (mt >= 0 && mt != j)) continue;
                    const double rest = mt == j ? ct[q] : ct[q] - g * (g > 0.0 ? lo0 : hi0);
                    double b = (ch[q] - rest) / g;
                    if (g > 0.0) {
                        if (isint) b = floor(b + 1e-6);
                        if (b < hi - 1e-9 * fmax(1.0, fabs(b))) hi = b;
                    } else {
                        if (isint) b = ceil(b - 1e-6);
                        if (b > lo + 1e-9 * fmax(1.0, fabs(b))) lo = b;
                    }
                }
            }
            if (lo > hi + 1e-6 * fmax(1.0, fabs(lo))) flag = 2.0;
            if (hi < lo) { if (hi0 == hi) lo = hi; else hi = lo; }      // (round-off: the bound that moved gives way)
            if (lo != lo0 || hi != hi0) { flag = fmax(flag, 1.0); w.clo[j] = lo; w.chi[j] = hi; }      // (only this thread reads column j's bounds in this phase)
        }
        const double f = block_max(sh, flag);
        if (f > 1.0) { ok = false; break; }
        if (f < 1.0) break;
    }
    __syncthreads();
    if (ok) for (int k = tid; k < w.nb; k += SOL_NT) { const int j = w.bins[k]; w.lo[j] = w.clo[j]; w.hi[j] = w.chi[j]; }
    __syncthreads();
    return ok;
}

// Rows that cannot bind under the ROOT bounds (largest activity <= right-hand side): their slack is basic in the slack basis,
// never violates its bound and so never leaves; nothing ever reads such a row again (cuts substitute rows of basic
// STRUCTURALS, verification goes to the original rows), so the pivots need not maintain it.  Marked once per instance
// in bit 1 of skip[] (the row index of a slack that never leaves stays its own).  Bounds only tighten below the root.
__device__ void s_mark_dead(const Ws &w, Shared &sh, bool enable, const double *act_pre, const ProblemDev *Psp, int mdl)
{
    const int n = w.n, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    for (int i = threadIdx.x; i < w.mcap; i += SOL_NT) w.skip[i] = 0;
    __syncthreads();
    // a row without a right-hand side (the standard constraint block switched off and no other block covers it: mld_set_std_block) does not exist
    for (int i = threadIdx.x; i < w.m0; i += SOL_NT) if (w.hs[i] >= 1.0e29) w.skip[i] = 2;
    __syncthreads();
    if (enable && Psp) {
        // after s_presolve: the largest activity of every row under the instance's implied bounds (w.clo / w.chi; the binaries' are the LP's), a thread per
        // row over the sparse copy
        const int *rp = Psp->csr_ptr + (size_t)mdl * (w.m0 + 1);
        const unsigned short *rc = Psp->csr_col + (size_t)mdl * Psp->nnz_cap;
        const double *rv = Psp->csr_val + (size_t)mdl * Psp->nnz_cap;
        for (int i = threadIdx.x; i < w.m0; i += SOL_NT) {
            double act = 0.0; bool inf = false;
            const int e1 = rp[i + 1];
            if (w.dbg & MLD_DBG_WALKS_SERIAL)
            for (int e = rp[i]; e < e1; ++e) {
                const int j = rc[e]; const double g = rv[e];
                const double b = g > 0.0 ? w.chi[j] : w.clo[j];
                if (fabs(b) >= 0.5 * S_BIG) inf = true; else act += g * b;
            }
            else {
                glb_cu16 *grc = (glb_cu16 *)rc; glb_cf64 *grv = (glb_cf64 *)rv, *glo = (glb_cf64 *)w.clo, *ghi = (glb_cf64 *)w.chi;
                for (int e = rp[i]; e < e1; e += WALK_GROUP) {
                    int cj[WALK_GROUP]; double cg[WALK_GROUP], cb[WALK_GROUP];
#pragma unroll
                    for (int q = 0; q < WALK_GROUP; ++q) { const int eq = min(e + q, e1 - 1); cj[q] = grc[eq]; cg[q] = grv[eq]; }
#pragma unroll
                    for (int q = 0; q < WALK_GROUP; ++q) cb[q] = cg[q] > 0.0 ? ghi[cj[q]] : glo[cj[q]];
#pragma unroll
                    for (int q = 0; q < WALK_GROUP; ++q) if (e + q < e1) { if (fabs(cb[q]) >= 0.5 * S_BIG) inf = true; else act += cg[q] * cb[q]; }
                }
            }
            if (!inf && act <= w.hs[i] - 1e-7) w.skip[i] = 2;
        }
    } else if (enable && act_pre) {
        // the bounds are the model's (no per-instance fixings): the largest activity of every row was computed once per model (round 3: the
        // per-instance scan below walked the model's 2.3 MB of rows with one dependent load per iteration -- 0.6 ms of the 1.1 ms set-up)
        for (int i = threadIdx.x; i < w.m0; i += SOL_NT) if (act_pre[i] <= w.hs[i] - 1e-7) w.skip[i] = 2;      // (also true for a row without right-hand side whenever its activity is bounded)
    } else if (enable)
    for (int i = wave; i < w.m0; i += SOL_NW) {
        const glb_f64 *g = (const glb_f64 *)(w.Gs + (size_t)i * n);
        const int jmax = w.nc_step > 0 ? min(n, (i / w.nc_step + 1) * w.nv_step) : n;     // causal rows (see s_mir_phase_a)
        double act = 0.0; int inf = 0;
        for (int j0 = 0; j0 < jmax; j0 += 256) {       // four independent loads in flight per lane
            double gq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int j = j0 + q * 64 + lane; gq[q] = j < jmax ? g[j] : 0.0; }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = j0 + q * 64 + lane;
                const double gj = gq[q];
                if (gj > 0.0) { const double hi = w.hi[j]; if (hi < 0.5 * S_BIG) act += gj * hi; else inf = 1; }
                else if (gj < 0.0) { const double lo = w.lo[j]; if (lo > -0.5 * S_BIG) act += gj * lo; else inf = 1; }
            }
        }
        act = wave_sum(act); act = __shfl(act, 0, 64);
        const bool any_inf = __ballot(inf) != 0ull;
        if (lane == 0 && !any_inf && act <= w.hs[i] - 1e-7) w.skip[i] = 2;
    }
    __syncthreads();
    int nl = 0;                             // the rows that are still maintained, ascending (reset / refresh / verification walk this list)
    for (int i0 = 0; i0 < w.m0; i0 += SOL_NT) {
        const int i = i0 + threadIdx.x;
        nl = block_compact(sh, i < w.m0 && !(w.skip[i] & 2), (unsigned short)i, w.live, nl);
    }
    __syncthreads();
    if (threadIdx.x == 0) sh.nlive = nl;
    __syncthreads();
    MLD_CHECK(w, nl <= w.m0, 138, nl, w.m0);
#ifdef MLD_ASSERT
    for (int t = threadIdx.x; t < nl; t += SOL_NT) MLD_CHECK(w, (int)w.live[t] < w.m0, 139, t, w.live[t]);
#endif
}

// stage marker for post-mortem diagnostics (mld_debug_trace): slot 1 = stage code, slot 2 = pivots so far; written through to host memory
#define MLD_MARK(w_, sh_, code_) do { if ((w_).trace && threadIdx.x == 0) { (w_).trace[1] = (code_); (w_).trace[2] = (sh_).pivots; __threadfence_system(); } } while (0)

// t-th maintained row of the dictionary: the live original rows, then the cut rows
__device__ __forceinline__ int live_row(const Ws &w, const Shared &sh, int t) { return t < sh.nlive ? (int)w.live[t] : w.m0 + (t - sh.nlive); }
__device__ __forceinline__ int live_count(const Ws &w, const Shared &sh) { return sh.nlive + (sh.m - w.m0); }

__device__ void s_reset_dictionary(const Ws &w, Shared &sh)
{
    const int n = w.n, ld = w.ld, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int nl = live_count(w, sh);
    // the slack basis first: the sparse fill below addresses a structural's column through where[]
    for (int i = tid; i < w.mcap; i += SOL_NT) { w.basic[i] = n + i; w.where[n + i] = -1 - i; }
    for (int c = tid; c < n; c += SOL_NT) { const int j = w.colperm[c]; w.nonbasic[c] = j; w.where[j] = c; }
    __syncthreads();
    // (round 4) with the sparse copy of the rows an ORIGINAL row is zero-filled (stores only: no load-to-store chain per row) and its 11 entries on average are
    // scattered into it afterwards; without it, and for the cut rows, the dense copy as before
    const int t_dense = w.csr_ptr ? sh.nlive : 0;
    for (int t = wave; t < nl; t += SOL_NW) {
        const int i = live_row(w, sh, t);
        double *dst = w.D + (size_t)i * ld;
        if (t < t_dense) {
            glb_f64 *dg = (glb_f64 *)dst;
            for (int k = lane; k < n; k += 64) dg[k] = 0.0;
            if (lane == 0) dst[n] = w.hs[i];
            continue;
        }
        const double *src = orig_row(w, i);
        if (i < w.m0 && w.Gp) {
            // eight independent 64-wide loads in flight before the first store (one load per iteration costs a full memory latency each)
            const glb_f64 *sp = (const glb_f64 *)(w.Gp + (size_t)i * n);
            glb_f64 *dg = (glb_f64 *)dst;
            for (int k0 = 0; k0 < n; k0 += 512) {
                double v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) { const int k = k0 + q * 64 + lane; v[q] = k < n ? sp[k] : 0.0; }
#pragma unroll
                for (int q = 0; q < 8; ++q) { const int k = k0 + q * 64 + lane; if (k < n) dg[k] = v[q]; }
            }
        }
        else for (int k = lane; k < n; k += 64) dst[k] = src[w.colperm[k]];
        if (lane == 0) dst[n] = orig_rhs(w, i);
    }
    double *d = w.dcost;
    for (int k = tid; k < n; k += SOL_NT) d[k] = w.qs[w.colperm[k]];
    if (tid == 0) d[n] = 0.0;
    __syncthreads();
    if (t_dense > 0) {
        for (int t = tid; t < t_dense; t += SOL_NT) {
            const int i = w.live[t];
            double *dst = w.D + (size_t)i * ld;
            const int e1 = w.csr_ptr[i + 1];
            if (w.dbg & MLD_DBG_WALKS_SERIAL) { for (int e = w.csr_ptr[i]; e < e1; ++e) dst[w.where[w.csr_col[e]]] = w.csr_val[e]; }
            else {
                glb_cu16 *rc = (glb_cu16 *)w.csr_col; glb_cf64 *rv = (glb_cf64 *)w.csr_val; glb_ci32 *wh = (glb_ci32 *)w.where;
                glb_f64 *dg = (glb_f64 *)dst;
                for (int e = w.csr_ptr[i]; e < e1; e += WALK_GROUP) {       // (a row's entries have distinct columns: the stores of a group do not meet)
                    int cj[WALK_GROUP], cc[WALK_GROUP]; double cg[WALK_GROUP];
#pragma unroll
                    for (int q = 0; q < WALK_GROUP; ++q) { const int eq = min(e + q, e1 - 1); cj[q] = rc[eq]; cg[q] = rv[eq]; }
#pragma unroll
                    for (int q = 0; q < WALK_GROUP; ++q) cc[q] = wh[cj[q]];
#pragma unroll
                    for (int q = 0; q < WALK_GROUP; ++q) if (e + q < e1) dg[cc[q]] = cg[q];
                }
            }
        }
        __syncthreads();
    }
}

// x_B of the slack basis right after s_reset_dictionary and the placement of the non-basic columns: x_B[i] = h_i - g_i . x_N over the sparse copy of the
// original rows (a thread per row) instead of a pass over the dictionary; only valid while no cut row exists and nothing has been pivoted
__device__ void s_refresh_initial(const Ws &w, Shared &sh)
{
    __syncthreads();
    for (int t = threadIdx.x; t < sh.nlive; t += SOL_NT) {
        const int i = w.live[t];
        double acc = w.hs[i];
        const int e1 = w.csr_ptr[i + 1];
        if (w.dbg & MLD_DBG_WALKS_SERIAL) { for (int e = w.csr_ptr[i]; e < e1; ++e) acc -= w.csr_val[e] * w.xN[w.where[w.csr_col[e]]]; }
        else {
            glb_cu16 *rc = (glb_cu16 *)w.csr_col; glb_cf64 *rv = (glb_cf64 *)w.csr_val; glb_ci32 *wh = (glb_ci32 *)w.where;
            for (int e = w.csr_ptr[i]; e < e1; e += WALK_GROUP) {
                int cj[WALK_GROUP], cc[WALK_GROUP]; double cg[WALK_GROUP], xv[WALK_GROUP];
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) { const int eq = min(e + q, e1 - 1); cj[q] = rc[eq]; cg[q] = rv[eq]; }
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) cc[q] = wh[cj[q]];
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) xv[q] = w.xN[cc[q]];
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) if (e + q < e1) acc -= cg[q] * xv[q];
            }
        }
        w.xB[i] = acc;
    }
    __syncthreads();
}

__device__ void s_refresh(const Ws &w, Shared &sh)
{   // xB = beta - D xN for all rows (xN staged in LDS, 4 rows per wave at a time)
    const int n = w.n, ld = w.ld, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = sh.m;
    lds_f64 *xs = (lds_f64 *)w.dabuf;
    const glb_f64 *D = (const glb_f64 *)w.D;
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += SOL_NT) xs[c] = w.xN[c];
    __syncthreads();
    const int nl = live_count(w, sh);
    (void)m;
    for (int t0 = wave * 4; t0 < nl; t0 += SOL_NW * 4) {
        const glb_f64 *rp[4]; int ri[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { ri[q] = live_row(w, sh, t0 + q < nl ? t0 + q : t0); rp[q] = D + (size_t)ri[q] * ld; }
        double s[4];
        wave_rows_dot4(rp[0], rp[1], rp[2], rp[3], xs, n, lane, s, (w.dbg & MLD_DBG_WALKS_SERIAL) != 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double t = wave_sum(s[q]);
            if (lane == 0 && t0 + q < nl) w.xB[ri[q]] = rp[q][n] - t;
        }
    }
    __syncthreads();
}

__device__ double s_objective_nosync(const Ws &w)
{   // debugging only: serial evaluation by the calling thread
    const double *d = w.dcost;
    double s = d[w.n];
    for (int c = 0; c < w.n; ++c) s += d[c] * w.xN[c];
    return s;
}

__device__ double s_objective(const Ws &w, Shared &sh)
{
    const double *d = w.dcost;
    double s = 0.0;
    for (int c = threadIdx.x; c < w.n; c += SOL_NT) s += d[c] * w.xN[c];
    return block_sum(sh, s) + d[w.n];
}

// A row that is not maintained (bit 1 of skip[]: it can never bind, s_mark_dead, or it is a cut row that s_purge_slack_cuts retired): the pivots leave its
// dictionary entries stale, its basic variable is its slack for good, and nobody reads its x_B -- pricing passes it over, s_refresh and the residual check
// do not compute it for an original row, s_gather_x reads x_B of basic structurals only.  A bound change therefore has nothing to update there
// (s_set_bounds, s_set_bounds_list; s_loop_flips skips these rows too).  skip[] through its LDS view where the shape placed it there.
__device__ __forceinline__ bool s_row_dead(const Ws &w, int r) { return ((w.all_lds ? ((const lds_u8 *)w.skip)[r] : w.skip[r]) & 2) != 0; }

// x_B -= D[:, c] * dl over the maintained rows, a thread per row: the gathers of two rows per thread are issued before the first use
__device__ __forceinline__ void s_bound_step(const Ws &w, const Shared &sh, int c, double dl)
{
    const glb_f64 *Dg = (const glb_f64 *)w.D;
    const int m = sh.m, ld = w.ld;
    for (int r0 = threadIdx.x; r0 < m; r0 += 2 * SOL_NT) {
        const int r1 = r0 + SOL_NT;
        const bool k0 = !s_row_dead(w, r0), k1 = r1 < m && !s_row_dead(w, r1);
        double v0 = 0.0, v1 = 0.0;
        if (k0) v0 = Dg[(size_t)r0 * ld + c];
        if (k1) v1 = Dg[(size_t)r1 * ld + c];
        if (k0) w.xB[r0] -= v0 * dl;
        if (k1) w.xB[r1] -= v1 * dl;
    }
}

// change the bounds of variable j keeping dual feasibility (all threads call)
__device__ void s_set_bounds(const Ws &w, Shared &sh, int j, double lo, double hi)
{
    const long long tb0 = wall_clock64();
    __syncthreads();
    MLD_CHECK(w, j >= 0 && j < w.n + w.mcap, 112, j, 0);
    const int c = w.where[j];
    MLD_CHECK(w, c < w.n && -1 - c < w.mcap, 112, j, c);
    double dl = 0.0;
    if (c >= 0) {
        const double old = w.xN[c];
        const double dc = w.dcost[c];
        double nw; unsigned char up;
        if (lo == hi) { nw = lo; up = 0; }
        else if (dc >= 0) { nw = lo; up = 0; }
        else { nw = hi; up = 1; }
        dl = nw - old;
        __syncthreads();
        if (threadIdx.x == 0) { w.xN[c] = nw; w.at_upper[c] = up; }
    }
    if (threadIdx.x == 0) { w.lo[j] = lo; w.hi[j] = hi; }
    if (c >= 0 && dl != 0.0) {
        if (w.dbg & MLD_DBG_DEAD_WORK_R8) { for (int r = threadIdx.x; r < sh.m; r += SOL_NT) w.xB[r] -= w.D[(size_t)r * w.ld + c] * dl; }      // (every row, as before: A/B)
        else s_bound_step(w, sh, c, dl);
    }
    __syncthreads();
    if (threadIdx.x == 0) sh.prof[4] += wall_clock64() - tb0;
}

// ordered rank of the flagged threads of one SOL_NT-wide chunk: *rank = number of flagged threads with a smaller index
// (valid where flag), returns the chunk's total
__device__ __forceinline__ int block_rank(Shared &sh, bool flag, int *rank)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    __syncthreads();
    if (lane == 0) sh.red_i[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < SOL_NW; ++q) { const int cq = sh.red_i[q]; if (q < wave) off += cq; tot += cq; }
    *rank = off + __popcll(bal & ((1ull << lane) - 1ull));
    return tot;
}

// s_set_bounds for a list of DISTINCT variables in one pass (leaves, RINS fixings, unwinding the stack): bounds and
// non-basic values are set in parallel, the moved columns are compacted in list order and x_B takes ONE combined
// update  x_B -= D[:, moved] * delta  (a wave per row) instead of one barrier-separated column gather per variable.
__device__ void s_set_bounds_list(const Ws &w, Shared &sh, const int *js, const double *los, const double *his, int count)
{
    const long long tb0 = wall_clock64();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ld = w.ld;
    typedef __attribute__((address_space(3))) unsigned short l_u16;
    typedef __attribute__((address_space(3))) double l_f64;
    l_u16 *clist = (l_u16 *)w.rowlist;
    l_f64 *dlist = (l_f64 *)w.colc;
    const double *d = w.dcost;
    const int chunk = w.mcap < SOL_NT ? w.mcap : ((w.mcap / SOL_NT) * SOL_NT);   // LDS lists hold mcap entries
    MLD_CHECK(w, count >= 0 && count <= w.nb + 2, 113, count, w.nb);
    for (int base = 0; base < count; base += chunk) {
        const int cnt = count - base < chunk ? count - base : chunk;
        __syncthreads();
        int nmove = 0;
        for (int k0 = 0; k0 < cnt; k0 += SOL_NT) {
            const int k = base + k0 + tid;
            bool mv = false; int c = -1; double delta = 0.0;
            if (k0 + tid < cnt) {
                const int j = js[k];
                const double lo = los[k], hi = his[k];
                MLD_CHECK(w, j >= 0 && j < w.n, 114, k, j);
                c = w.where[j];
                MLD_CHECK(w, c < w.n && -1 - c < w.mcap, 115, j, c);
                if (c >= 0) {
                    const double old = w.xN[c], dc = d[c];
                    double nw; unsigned char up;
                    if (lo == hi) { nw = lo; up = 0; }
                    else if (dc >= 0) { nw = lo; up = 0; }
                    else { nw = hi; up = 1; }
                    delta = nw - old;
                    w.xN[c] = nw; w.at_upper[c] = up;
                    mv = delta != 0.0;
                }
                w.lo[j] = lo; w.hi[j] = hi;
            }
            int rank;
            const int tot = block_rank(sh, mv, &rank);
            if (mv) { clist[nmove + rank] = (unsigned short)c; dlist[nmove + rank] = delta; }
            nmove += tot;
        }
        __syncthreads();
        if (nmove > 0 && !(w.dbg & (MLD_DBG_WALKS_SERIAL | MLD_DBG_DEAD_WORK_R8))) {
            // The maintained rows only (s_row_dead): the grouping below over the list of maintained rows (live_row) instead of over every row, so a
            // third fewer groups on the bench shape.  The list holds every cut row: one that was retired keeps its slot in a group -- its gathers are
            // still issued (a stale row, read and not used), only its x_B is neither loaded nor stored, like a row past the end; such rows are few, and
            // compacting them out would cost an exchange per call.  The four row indices of the NEXT group are read while this one's gathers are in
            // flight.  Per row the same sum over the same lanes in the same order.
            const glb_f64 *Dg = (const glb_f64 *)w.D;
            const int nl = live_count(w, sh), nlive = sh.nlive;
            int ri[4], rn[4]; bool rk[4], kn[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int t = wave + q * SOL_NW, r = __builtin_amdgcn_readfirstlane(live_row(w, sh, t < nl ? t : 0));      // (the same in every lane of the wave)
                ri[q] = r; rk[q] = t < nl && !(t >= nlive && s_row_dead(w, r));
            }
            for (int t0 = wave; t0 < nl; t0 += 4 * SOL_NW) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int t = t0 + (4 + q) * SOL_NW, r = __builtin_amdgcn_readfirstlane(live_row(w, sh, t < nl ? t : 0));
                    rn[q] = r; kn[q] = t < nl && !(t >= nlive && s_row_dead(w, r));
                }
                double sa[4] = {0.0, 0.0, 0.0, 0.0}, xb[4];
                for (int tb = 0; tb < nmove; tb += 64) {
                    const int t = tb + lane; const bool ok = t < nmove;
                    const int c = ok ? (int)clist[t] : 0; const double dl = ok ? dlist[t] : 0.0;
                    double v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = Dg[(size_t)ri[q] * ld + c];      // (no branch: a lane past the list reads column 0, a slot without a row reads a maintained row; neither is used)
#pragma unroll
                    for (int q = 0; q < 4; ++q) if (ok) sa[q] += v[q] * dl;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) xb[q] = (lane == 0 && rk[q]) ? w.xB[ri[q]] : 0.0;
                for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) sa[q] += __shfl_down(sa[q], o, 64);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) if (lane == 0 && rk[q]) w.xB[ri[q]] = xb[q] - sa[q];
#pragma unroll
                for (int q = 0; q < 4; ++q) { ri[q] = rn[q]; rk[q] = kn[q]; }
            }
        } else if (nmove > 0 && !(w.dbg & MLD_DBG_WALKS_SERIAL)) {
            // (every row, as before: A/B) a wave takes four rows at a time (r, r + SOL_NW, ...): the gathers of all four are issued together, their shuffle sums run interleaved, then
            // the four stores; per row the same sum over the same lanes as the loop below (a row past the end of a tail group adds zeros and stores nothing)
            const glb_f64 *Dg = (const glb_f64 *)w.D;
            const int m = sh.m;
            for (int r0 = wave; r0 < m; r0 += 4 * SOL_NW) {
                double sa[4] = {0.0, 0.0, 0.0, 0.0}, xb[4];
                for (int tb = 0; tb < nmove; tb += 64) {
                    const int t = tb + lane; const bool ok = t < nmove;
                    const int c = ok ? (int)clist[t] : 0; const double dl = ok ? dlist[t] : 0.0;
                    double v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { const int r = r0 + q * SOL_NW < m ? r0 + q * SOL_NW : r0; v[q] = Dg[(size_t)r * ld + c]; }      // (no branch: a lane past the list reads column 0, a row past the end row r0 again; neither is used)
#pragma unroll
                    for (int q = 0; q < 4; ++q) if (ok) sa[q] += v[q] * dl;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) { const int r = r0 + q * SOL_NW; xb[q] = (lane == 0 && r < m) ? w.xB[r] : 0.0; }
                for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) sa[q] += __shfl_down(sa[q], o, 64);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) { const int r = r0 + q * SOL_NW; if (lane == 0 && r < m) w.xB[r] = xb[q] - sa[q]; }
            }
        } else if (nmove > 0)
            for (int r = wave; r < sh.m; r += SOL_NW) {
                if (!(w.dbg & MLD_DBG_DEAD_WORK_R8) && s_row_dead(w, r)) continue;
                const double *row = w.D + (size_t)r * ld;
                double sacc = 0.0;
                for (int t = lane; t < nmove; t += 64) sacc += row[clist[t]] * dlist[t];
                sacc = wave_sum(sacc);
                if (lane == 0) w.xB[r] -= sacc;
            }
    }
    __syncthreads();
    if (tid == 0) sh.prof[4] += wall_clock64() - tb0;
}

// Explicit address spaces: the workspace view (Ws) holds generic pointers, which compile to flat_* accesses that
// couple the vector-memory and LDS counters.  Hot loops cast them back once: LDS -> ds_read/ds_write, HBM -> global_*.

// Rows `rowlist[0..nrows)` -= colc[row] * (scaled pivot row) on the sector groups g0 .. g0+NG-1 (16 sectors = 1 KiB each).
// A lane moves 16 bytes (4 lanes per 64-byte sector); a wave takes RB rows at a time, so RB*NG independent 1 KiB
// loads (up to 32 KiB per wave, 256 KiB per CU) are in flight before the first use -- the loop is latency-bound.
#ifndef SOL_SEC
#define SOL_SEC 8            // doubles per update sector (8 = 64 bytes)
#endif
#define SOL_LPS (SOL_SEC / 2) // lanes per sector (16 bytes each)
#define SOL_SPW (64 / SOL_LPS) // sectors per wave instruction
// One element of the rank-1 update, o - mu * rr, as ONE fused multiply-add.  The update of the rows (s_update_rows, s_update_rows2), the look-ahead's ratio-test row
// (s_look_ahead) and the second pivot's multiplier column (s_pivot_head) all go through here: an entry has the same bits whichever of them computes it.
__device__ __forceinline__ double s_upd(double o, double mu, double rr) { return __builtin_fma(-mu, rr, o); }

// rows a wave takes at a time when a chunk has ng groups of sectors: the ONE definition (the four update templates; mld_debug_update_shape reports it)
__host__ __device__ constexpr int s_update_rb(int ng) { return (ng <= 2 ? 16 : (ng == 3 ? 10 : 8)) / (SOL_WPE / 2); }

template <int NG>
__device__ __forceinline__ void s_update_rows(glb_f64 *D, int ld, const lds_f64 *rowr, const lds_f64 *colc, const lds_u16 *rowlist,
                                              const lds_u16 *seclist, int nrows, int nact, int g0, int c, int wave, int lane)
{
    constexpr int RB = s_update_rb(NG);
    const int sub = lane / SOL_LPS, pr = (lane % SOL_LPS) * 2;
    int koff[NG]; bool ok[NG], cx[NG], cy[NG]; double2_t rr[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int si = (g0 + g) * SOL_SPW + sub;
        ok[g] = si < nact;
        koff[g] = ok[g] ? (int)seclist[si] * SOL_SEC + pr : 0;      // k and k+1 lie inside the row (ld is a multiple of 8)
        rr[g] = ok[g] ? *(const lds_f64x2 *)(rowr + koff[g]) : (double2_t){0.0, 0.0};
        cx[g] = ok[g] && koff[g] == c; cy[g] = ok[g] && koff[g] + 1 == c;   // entering column: old entry counts as 0 (rowr[c] = 1/p)
    }
    for (int b = wave * RB; b < nrows; b += SOL_NW * RB) {
        double2_t v[RB][NG];
        int rowi[RB];
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            rowi[q] = b + q < nrows ? __builtin_amdgcn_readfirstlane((int)rowlist[b + q]) : -1;
            if (rowi[q] >= 0) {
                const glb_f64 *base = D + (size_t)rowi[q] * ld;
#pragma unroll
                for (int g = 0; g < NG; ++g) v[q][g] = ok[g] ? *(const glb_f64x2 *)(base + koff[g]) : (double2_t){0.0, 0.0};
            }
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            if (rowi[q] >= 0) {
                const double mu = colc[rowi[q]];
                glb_f64 *base = D + (size_t)rowi[q] * ld;
#pragma unroll
                for (int g = 0; g < NG; ++g)
                    if (ok[g]) {
                        double2_t o = v[q][g];
                        if (cx[g]) o.x = 0.0;
                        if (cy[g]) o.y = 0.0;
                        o.x = s_upd(o.x, mu, rr[g].x); o.y = s_upd(o.y, mu, rr[g].y);
                        *(glb_f64x2 *)(base + koff[g]) = o;
                    }
            }
        }
    }
}

// The updates of TWO consecutive pivots in one pass (s_pivot_pair): rows `rowlist` (the union of both pivots' rows, without the second pivot's row) on the sectors
// `seclist` (the union of both pivot rows' active sectors; secflag[sector] bit 0 = active in the first row, bit 1 = in the second).  A (row, sector) pair is loaded
// once, takes the first pivot's update if the row has a non-zero first multiplier and the sector is active in the first row, then the second pivot's likewise -- each
// with its own entering column counted as 0 -- and is stored once; a pair that belongs to neither pivot is not touched.  Every element goes through the same
// operations in the same order as in two separate passes.
template <int NG>
__device__ __forceinline__ void s_update_rows2(glb_f64 *D, int ld, const lds_f64 *rowr1, const lds_f64 *colc1, const lds_f64 *rowr2, const lds_f64 *colc2,
                                               const lds_u16 *rowlist, const lds_u16 *seclist, const lds_u8 *secflag, int nrows, int nact, int g0,
                                               int r1, int c1, int c2, int wave, int lane)
{
    constexpr int RB = s_update_rb(NG);
    const int sub = lane / SOL_LPS, pr = (lane % SOL_LPS) * 2;
    int koff[NG]; bool a1[NG], a2[NG], cx1[NG], cy1[NG], cx2[NG], cy2[NG]; double2_t rr1[NG], rr2[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int si = (g0 + g) * SOL_SPW + sub;
        const bool ok = si < nact;
        const int sec = ok ? (int)seclist[si] : 0;
        const int fl = ok ? (int)secflag[sec] : 0;
        a1[g] = (fl & 1) != 0; a2[g] = (fl & 2) != 0;
        koff[g] = sec * SOL_SEC + pr;
        rr1[g] = a1[g] ? *(const lds_f64x2 *)(rowr1 + koff[g]) : (double2_t){0.0, 0.0};
        rr2[g] = a2[g] ? *(const lds_f64x2 *)(rowr2 + koff[g]) : (double2_t){0.0, 0.0};
        cx1[g] = koff[g] == c1; cy1[g] = koff[g] + 1 == c1;
        cx2[g] = koff[g] == c2; cy2[g] = koff[g] + 1 == c2;
    }
    for (int b = wave * RB; b < nrows; b += SOL_NW * RB) {
        double2_t v[RB][NG];
        int rowi[RB], rowf[RB];      // row and (wave-uniform) bit 0: it takes the first update, bit 1: the second
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            rowi[q] = b + q < nrows ? __builtin_amdgcn_readfirstlane((int)rowlist[b + q]) : -1;
            rowf[q] = 0;
            if (rowi[q] >= 0) {
                // (the first pivot's own row holds the pivot element in colc1, not a multiplier: it takes the second update only)
                rowf[q] = __builtin_amdgcn_readfirstlane((int)(rowi[q] != r1 && colc1[rowi[q]] != 0.0) | ((int)(colc2[rowi[q]] != 0.0) << 1));
                const bool f1 = rowf[q] & 1, f2 = rowf[q] & 2;
                const glb_f64 *base = D + (size_t)rowi[q] * ld;
#pragma unroll
                for (int g = 0; g < NG; ++g) v[q][g] = ((f1 && a1[g]) || (f2 && a2[g])) ? *(const glb_f64x2 *)(base + koff[g]) : (double2_t){0.0, 0.0};
            }
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            if (rowi[q] >= 0) {
                const bool f1 = rowf[q] & 1, f2 = rowf[q] & 2;
                const double mu1 = colc1[rowi[q]], mu2 = colc2[rowi[q]];
                glb_f64 *base = D + (size_t)rowi[q] * ld;
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const bool u1 = f1 && a1[g], u2 = f2 && a2[g];
                    if (u1 || u2) {
                        double2_t o = v[q][g];
                        if (u1) {
                            if (cx1[g]) o.x = 0.0;
                            if (cy1[g]) o.y = 0.0;
                            o.x = s_upd(o.x, mu1, rr1[g].x); o.y = s_upd(o.y, mu1, rr1[g].y);
                        }
                        if (u2) {
                            if (cx2[g]) o.x = 0.0;
                            if (cy2[g]) o.y = 0.0;
                            o.x = s_upd(o.x, mu2, rr2[g].x); o.y = s_upd(o.y, mu2, rr2[g].y);
                        }
                        *(glb_f64x2 *)(base + koff[g]) = o;
                    }
                }
            }
        }
    }
}

// ---- the same two updates with a unit (one row x one group of 16 sectors: a 16-byte load, the fused multiply-adds, a 16-byte store) close to its payload ----
// (s_update_rows_r7, s_update_rows2_r7: what the loop runs; MLD_DBG_UPDATE_R7 keeps the two templates above selectable in the legacy instantiation.  Every
// element sees the operations of the templates above in their order and is stored where they store it; what differs is where the exceptions are paid for.)
//  * A pivot's last group of 16 sectors is rarely full.  Its lanes past the last active sector repeat that sector: the same address, the same operands, the
//    same value stored -- no lane of a group is ever switched off, so no unit carries a test for it.
//  * The entering column belongs to one lane of one group.  That group trades places with the chunk's first (the second pivot's with the chunk's second), so
//    only slot 0 (and slot 1 for the second pivot) carries the two selects that count the old entry as 0.
//  * Rows go to the waves round robin (row t of a block of SOL_NW * RB to wave t % SOL_NW): 84 rows are 10 or 11 for each wave instead of 16 for five of them
//    and none for two.  The LOAD phase of a block has no control flow: a wave that has fewer than RB rows left loads its last row again in the remaining
//    slots (the same lines, read and never used), so all RB * NG loads are issued back to back before the first use, as in the templates above; a load under a
//    test of the row count made the compiler wait for the loads in flight before every row.  Only the compute phase tests the row count, a scalar branch per row.
//  * In the pair, the row's flags (first update, second, both) are wave-uniform: a branch picks one of three bodies instead of selects per lane and unit.
//  * What is the same in every lane is told to the compiler (S_UNI): the workspace view lives in private memory, so without it the leading dimension, the row
//    count and the wave's number count as per-lane values, every row test becomes a lane mask and every address a 64-bit vector sum.  With it a row's base is a
//    scalar pair; a unit's address is that pair plus the lane's byte offset.
#define S_UNI(x_) __builtin_amdgcn_readfirstlane(x_)
#ifndef MLD_UPDATE_LEGACY_ALWAYS
#define MLD_UPDATE_LEGACY_ALWAYS 0      // (-DMLD_UPDATE_LEGACY_ALWAYS=1: a measurement build whose default loop keeps the earlier templates, DESIGN section 6)
#endif
__device__ __forceinline__ glb_f64 *s_uni_ptr(glb_f64 *p)
{
    const unsigned long long v = (unsigned long long)p;
    return (glb_f64 *)(((unsigned long long)(unsigned)S_UNI((int)(v >> 32)) << 32) | (unsigned)S_UNI((int)v));
}
// (the empty asm keeps the 32-bit offset opaque up to its use: widened once outside the loop it is a register pair per group, and the access a 64-bit vector add
// plus `global_* v, v[a:b], off`; kept 32-bit it is `global_* v, v_off, s[base]`, one register and no add)
__device__ __forceinline__ double2_t s_ld16(const glb_f64 *base, unsigned off) { asm volatile("" : "+v"(off)); return *(const glb_f64x2 *)((const __attribute__((address_space(1))) char *)base + off); }
__device__ __forceinline__ void s_st16(glb_f64 *base, unsigned off, double2_t o) { asm volatile("" : "+v"(off)); *(glb_f64x2 *)((__attribute__((address_space(1))) char *)base + off) = o; }
// (true when one of the 16 sectors of group `grp` -- as this wave's lanes read them -- is sector `sec`; wave-uniform)
__device__ __forceinline__ bool s_group_holds(const lds_u16 *seclist, int nact, int grp, int sub, int sec)
{
    const int si = min(grp * SOL_SPW + sub, nact - 1);
    return __ballot((int)seclist[si] == sec) != 0ull;
}

template <int NG>
__device__ __forceinline__ void s_update_rows_r7(glb_f64 *D, int ld, const lds_f64 *rowr, const lds_f64 *colc, const lds_u16 *rowlist,
                                                 const lds_u16 *seclist, int nrows, int nact, int g0, int c, int wave, int lane)
{
    constexpr int RB = s_update_rb(NG);
    const int sub = lane / SOL_LPS, pr = (lane % SOL_LPS) * 2;
    D = s_uni_ptr(D); ld = S_UNI(ld); wave = S_UNI(wave); nrows = S_UNI(nrows); nact = S_UNI(nact); g0 = S_UNI(g0); c = S_UNI(c);
    int grp[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) grp[g] = g0 + g;
#pragma unroll
    for (int g = 1; g < NG; ++g)
        if (s_group_holds(seclist, nact, g0 + g, sub, c / SOL_SEC)) { grp[0] = g0 + g; grp[g] = g0; }
    unsigned koff[NG]; double2_t rr[NG];      // byte offset of the lane's 16 bytes in a row; the pivot row's two entries there
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int si = min(grp[g] * SOL_SPW + sub, nact - 1);
        const int k = (int)seclist[si] * SOL_SEC + pr;      // k and k+1 lie inside the row (ld is a multiple of 8)
        koff[g] = (unsigned)k * 8u;
        rr[g] = *(const lds_f64x2 *)(rowr + k);
    }
    const bool cx = koff[0] == (unsigned)c * 8u, cy = koff[0] + 8u == (unsigned)c * 8u;   // entering column: old entry counts as 0 (rowr[c] = 1/p)
    for (int b = wave; b < nrows; b += SOL_NW * RB) {
        const int nq = min(RB, (nrows - b + SOL_NW - 1) / SOL_NW);      // this wave's rows of the block: b, b + SOL_NW, ...
        double2_t v[RB][NG];
        int rowi[RB];
#pragma unroll
        for (int q = 0; q < RB; ++q) {      // (no branch in here: slots past the wave's last row repeat it)
            rowi[q] = S_UNI((int)rowlist[b + min(q, nq - 1) * SOL_NW]);
            const glb_f64 *base = D + (size_t)rowi[q] * ld;
#pragma unroll
            for (int g = 0; g < NG; ++g) v[q][g] = s_ld16(base, koff[g]);
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            if (q < nq) {
                const double mu = colc[rowi[q]];
                glb_f64 *base = D + (size_t)rowi[q] * ld;
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    double2_t o = v[q][g];
                    if (g == 0) { if (cx) o.x = 0.0; if (cy) o.y = 0.0; }
                    o.x = s_upd(o.x, mu, rr[g].x); o.y = s_upd(o.y, mu, rr[g].y);
                    s_st16(base, koff[g], o);
                }
            }
        }
    }
}

// one unit of the pair: the first pivot's update where A1, then the second's where A2 (compile-time: the row's wave-uniform flags), each on the lanes whose sector
// is active in that pivot's row; Z1 / Z2: the slot can hold that pivot's entering column
template <bool A1, bool A2, bool Z1, bool Z2>
__device__ __forceinline__ double2_t s_upd2_unit(double2_t o, bool a1, bool a2, double mu1, double mu2, double2_t rr1, double2_t rr2, bool cx1, bool cy1, bool cx2, bool cy2)
{
    if (A1 && a1) {
        if (Z1) { if (cx1) o.x = 0.0; if (cy1) o.y = 0.0; }
        o.x = s_upd(o.x, mu1, rr1.x); o.y = s_upd(o.y, mu1, rr1.y);
    }
    if (A2 && a2) {
        if (Z2) { if (cx2) o.x = 0.0; if (cy2) o.y = 0.0; }
        o.x = s_upd(o.x, mu2, rr2.x); o.y = s_upd(o.y, mu2, rr2.y);
    }
    return o;
}

// (A row of the union list is loaded on all its listed sectors, also where only one of its two updates applies and that pivot's row is not active in the sector:
// a load that depends on the lane's flags would make every register of the block conditionally defined, and the waits for them would end the loads in flight.
// Of the sector-rows of a pair 88 % belong to both pivots, DESIGN section 6; what is loaded for nothing is the corners of the union.  Stores are where they were.)
template <int NG>
__device__ __forceinline__ void s_update_rows2_r7(glb_f64 *D, int ld, const lds_f64 *rowr1, const lds_f64 *colc1, const lds_f64 *rowr2, const lds_f64 *colc2,
                                                  const lds_u16 *rowlist, const lds_u16 *seclist, const lds_u8 *secflag, int nrows, int nact, int g0,
                                                  int r1, int c1, int c2, int wave, int lane)
{
    constexpr int RB = s_update_rb(NG);
    const int sub = lane / SOL_LPS, pr = (lane % SOL_LPS) * 2;
    D = s_uni_ptr(D); ld = S_UNI(ld); wave = S_UNI(wave); nrows = S_UNI(nrows); nact = S_UNI(nact); g0 = S_UNI(g0); r1 = S_UNI(r1); c1 = S_UNI(c1); c2 = S_UNI(c2);
    int grp[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) grp[g] = g0 + g;
#pragma unroll
    for (int g = 1; g < NG; ++g)      // the first pivot's entering column to slot 0
        if (s_group_holds(seclist, nact, g0 + g, sub, c1 / SOL_SEC)) { grp[0] = g0 + g; grp[g] = g0; }
    if constexpr (NG > 2) {      // the second's to slot 1, unless slot 0 or 1 has it
#pragma unroll
        for (int g = 2; g < NG; ++g)
            if (s_group_holds(seclist, nact, grp[g], sub, c2 / SOL_SEC)) { const int t = grp[1]; grp[1] = grp[g]; grp[g] = t; }
    }
    unsigned koff[NG]; bool a1[NG], a2[NG]; double2_t rr1[NG], rr2[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int si = min(grp[g] * SOL_SPW + sub, nact - 1);
        const int sec = (int)seclist[si];
        const int fl = (int)secflag[sec];
        const int k = sec * SOL_SEC + pr;
        a1[g] = (fl & 1) != 0; a2[g] = (fl & 2) != 0;
        koff[g] = (unsigned)k * 8u;
        rr1[g] = a1[g] ? *(const lds_f64x2 *)(rowr1 + k) : (double2_t){0.0, 0.0};
        rr2[g] = a2[g] ? *(const lds_f64x2 *)(rowr2 + k) : (double2_t){0.0, 0.0};
    }
    constexpr int S1 = NG > 1 ? 1 : 0;      // the slot besides 0 that can hold the second entering column
    const unsigned b1 = (unsigned)c1 * 8u, b2 = (unsigned)c2 * 8u;
    const bool cx1 = koff[0] == b1, cy1 = koff[0] + 8u == b1, cx2 = koff[0] == b2, cy2 = koff[0] + 8u == b2;
    const bool dx2 = koff[S1] == b2, dy2 = koff[S1] + 8u == b2;
    for (int b = wave; b < nrows; b += SOL_NW * RB) {
        const int nq = min(RB, (nrows - b + SOL_NW - 1) / SOL_NW);
        double2_t v[RB][NG];
        int rowc[RB];      // (wave-uniform) the row
#pragma unroll
        for (int q = 0; q < RB; ++q) {      // (no branch in here: slots past the wave's last row repeat it)
            const int row = S_UNI((int)rowlist[b + min(q, nq - 1) * SOL_NW]);
            rowc[q] = row;
            const glb_f64 *base = D + (size_t)row * ld;
#pragma unroll
            for (int g = 0; g < NG; ++g) v[q][g] = s_ld16(base, koff[g]);
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            if (q < nq) {
                const int row = rowc[q];
                const double mu1 = colc1[row], mu2 = colc2[row];
                // (the first pivot's own row holds the pivot element in colc1, not a multiplier: it takes the second update only)
                const int f = S_UNI((int)(row != r1 && mu1 != 0.0) | ((int)(mu2 != 0.0) << 1));
                glb_f64 *base = D + (size_t)row * ld;
                if (f == 3) {      // (every listed sector is active in one of the two rows: every lane stores)
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        const double2_t o = g == 0 ? s_upd2_unit<true, true, true, true>(v[q][g], a1[g], a2[g], mu1, mu2, rr1[g], rr2[g], cx1, cy1, cx2, cy2)
                                          : g == S1 ? s_upd2_unit<true, true, false, true>(v[q][g], a1[g], a2[g], mu1, mu2, rr1[g], rr2[g], false, false, dx2, dy2)
                                                    : s_upd2_unit<true, true, false, false>(v[q][g], a1[g], a2[g], mu1, mu2, rr1[g], rr2[g], false, false, false, false);
                        s_st16(base, koff[g], o);
                    }
                } else if (f == 1) {
#pragma unroll
                    for (int g = 0; g < NG; ++g)
                        if (a1[g]) {
                            const double2_t o = g == 0 ? s_upd2_unit<true, false, true, false>(v[q][g], true, false, mu1, mu2, rr1[g], rr2[g], cx1, cy1, false, false)
                                                       : s_upd2_unit<true, false, false, false>(v[q][g], true, false, mu1, mu2, rr1[g], rr2[g], false, false, false, false);
                            s_st16(base, koff[g], o);
                        }
                } else if (f == 2) {
#pragma unroll
                    for (int g = 0; g < NG; ++g)
                        if (a2[g]) {
                            const double2_t o = g == 0 ? s_upd2_unit<false, true, false, true>(v[q][g], false, true, mu1, mu2, rr1[g], rr2[g], false, false, cx2, cy2)
                                              : g == S1 ? s_upd2_unit<false, true, false, true>(v[q][g], false, true, mu1, mu2, rr1[g], rr2[g], false, false, dx2, dy2)
                                                        : s_upd2_unit<false, true, false, false>(v[q][g], false, true, mu1, mu2, rr1[g], rr2[g], false, false, false, false);
                            s_st16(base, koff[g], o);
                        }
                }
            }
        }
    }
}

// First half of a pivot (entering column c, leaving row r, leaving variable goes to leave_value): everything but the update of the other rows.  The multiplier column
// and the pivot row are staged in LDS (colc, rowr); the row is scaled (LDS and dictionary); x_B, the devex weights, the cost row and the basis maps move on.  All of
// that reads only the staged row and column and the small per-basis arrays, so the update of the other rows is the LAST thing a pivot does (s_pivot_inl) and the
// next pivot can be chosen before it (s_pivot_pair).
// SECOND: the pivot follows one whose row update has not been done yet (its row r1 and column c1 are staged in w.rowr / w.colc, w.secflag bit 0 marks its active
// sectors).  rowr already holds row r as that update leaves it (s_look_ahead); the column's entries get the same correction.
// Three block barriers: (1) on entry -- the ratio test's readers of the staging buffers (ea[cbest]) are done; (2) after the staging -- the pivot element, which the
// thread that staged it left in sh.piv_el, and everything read before it (x_B[r], x_N[c], w[r], d[c]) is in every thread's registers before any of them is written;
// (3) at the end.  Between (2) and (3) no thread reads what another one writes: a thread scales the rowr[k] and reads the colc[i] it staged itself, updates its own
// x_B[i], w[i] (the owner of row r writes the entering value) and d[k] from the rowr[k] it scaled (the owner of column n takes d[n]), and thread 0's book-keeping
// touches scalars nobody reads before (3).  MLD_DBG_PIVOT_SYNC_R5 puts the three barriers that stood between these steps back (DESIGN section 6: hazard table).
template <bool L, bool SECOND, bool LEG>
__device__ __forceinline__ void s_pivot_head(const Ws &w, Shared &sh, int r, int c, double leave_value, lds_f64 *rowr, lds_f64 *colc, int r1, int c1)
{
    HOT_VIEW(L, w);
    const int n = w.n, ld = w.ld, m = sh.m, tid = threadIdx.x;
    glb_f64 *D = (glb_f64 *)w.D;
    glb_f64 *rowr_g = D + (size_t)r * ld;
    MLD_CHECK(w, r >= 0 && r < m && c >= 0 && c < n && m <= w.mcap, 101, r, c);
    const bool sync_r5 = LEG && (w.dbg & MLD_DBG_PIVOT_SYNC_R5) != 0;      // the three barriers this function no longer needs (below), kept selectable (legacy instantiation)
    __syncthreads();
    // stage multiplier column and the pivot row in LDS (raw first: the pivot element goes to sh.piv_el)
    if (!SECOND) {   // (rows that can never bind are not maintained: multiplier 0.)  All loads of both gathers are issued before the first LDS store: the
        // column gather is one 64-byte sector per element and each dependent round costs a full memory latency
        const int span = (m > n + 1 ? m : n + 1);
        for (int b0 = 0; b0 < span; b0 += 4 * SOL_NT) {
            double cv[4], rv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = b0 + q * SOL_NT + tid;
                cv[q] = (i < m && !(h_skip[i] & 2)) ? D[(size_t)i * ld + c] : 0.0;
                rv[q] = (i <= n) ? rowr_g[i] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = b0 + q * SOL_NT + tid;
                if (i < m) colc[i] = cv[q];
                if (i <= n) rowr[i] = rv[q];
                if (i == c) sh.piv_el = rv[q];
            }
        }
    } else {
        const lds_f64 *rowr1 = (const lds_f64 *)w.rowr, *colc1 = (const lds_f64 *)w.colc;
        const bool act1 = (((const lds_u8 *)w.secflag)[c / SOL_SEC] & 1) != 0;      // the pending update touches column c (of the rows with a non-zero multiplier)
        const double rr = rowr1[c];
        for (int b0 = 0; b0 < m; b0 += 4 * SOL_NT) {
            double cv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = b0 + q * SOL_NT + tid;
                cv[q] = (i < m && !(h_skip[i] & 2)) ? D[(size_t)i * ld + c] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = b0 + q * SOL_NT + tid;
                if (i >= m) continue;
                double v = cv[q];
                if (i == r1) v = rr;                                  // the first pivot's row is the scaled row
                else {
                    const double mu = colc1[i];                       // (0 for a row that is not maintained)
                    if (act1 && mu != 0.0) v = s_upd(c == c1 ? 0.0 : v, mu, rr);
                }
                colc[i] = v;
            }
        }
        if (tid == c % SOL_NT) sh.piv_el = rowr[c];      // (s_look_ahead staged rowr[c] on this thread)
    }
    typename HotT<L>::f64p d = h_d;    // cost row: LDS when it fits (SolverShape::lCost), else the row after the last dictionary row
    const double xBr = h_xB[r], xNc = h_xN[c], wr = h_dw[r], dc = d[c];
    __syncthreads();
    const double p = sh.piv_el;
    const double inv = 1.0 / p;
    const double theta = (xBr - leave_value) * inv;
    const double enter_val = xNc + theta;
    if (sync_r5) __syncthreads();
    int my_nz = 0;
    for (int k = tid; k <= n; k += SOL_NT) { const double v = (k == c) ? inv : rowr[k] * inv; rowr[k] = v; rowr_g[k] = v; my_nz += (v != 0.0); }
    if (w.dbg && my_nz) atomicAdd((unsigned long long *)&sh.prof[7], (unsigned long long)my_nz);   // pivot-row non-zeros (diagnostic)
    for (int i = tid; i < m; i += SOL_NT) {
        const double ci = colc[i];
        // devex (oracle pivot()): w_i = max(w_i, (alpha_iq / alpha_rq)^2 w_r) on the touched rows, w_r = max(w_r / alpha_rq^2, 1)
        if (i == r) { h_xB[i] = enter_val; h_dw[i] = fmax(wr * inv * inv, 1.0); }      // (the entering variable takes the row over)
        else {
            h_xB[i] -= ci * theta;
            if (ci != 0.0) { const double f = ci * inv, c2 = f * f * wr; if (c2 > h_dw[i]) h_dw[i] = c2; }
        }
    }
    if (sync_r5) __syncthreads();
    {   // cost row: obj = d[n] + sum_c d_c xN_c
        if (tid == 0) sh.s_d[0] = dc * theta;      // objective change of this pivot (entering variable moves by theta)
        if (sync_r5) __syncthreads();
        if (dc != 0.0) {      // (every thread reads only the rowr[k] it scaled itself)
            for (int k = tid; k < n; k += SOL_NT) d[k] = (k == c) ? -dc * inv : d[k] - dc * rowr[k];
            if (tid == n % SOL_NT) d[n] += dc * rowr[n];
        }
    }
    if (tid == 0) {
        const int jb = h_basic[r], jn = h_nonbasic[c];
        MLD_CHECK(w, jb >= 0 && jb < n + w.mcap && jn >= 0 && jn < n + w.mcap, 109, jb, jn);
        h_basic[r] = jn; h_nonbasic[c] = jb;
        w.where[jn] = -1 - r; w.where[jb] = c;
        h_xN[c] = leave_value;
        h_up[c] = (leave_value == h_hi[jb]) && (h_lo[jb] != h_hi[jb]);
        sh.pivots++; sh.since_check++;
    }
    __syncthreads();
}

// Second half of a pivot whose first half s_pivot_head<L, false> has staged in w.rowr / w.colc: rows with a non-zero multiplier -= multiplier * (scaled pivot row) on
// the row's active sectors
template <bool LEG>
__device__ __forceinline__ void s_pivot_update(const Ws &w, Shared &sh, int r, int c, long long tp0)
{
    const int n = w.n, ld = w.ld, m = sh.m, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    glb_f64 *D = (glb_f64 *)w.D;
    lds_f64 *rowr = (lds_f64 *)w.rowr, *colc = (lds_f64 *)w.colc;
    lds_u16 *seclist = (lds_u16 *)w.seclist, *rowlist = (lds_u16 *)w.rowlist;
#ifdef MLD_PIVOT_PROF
    const long long tq1 = wall_clock64();
#endif
    // active 64-byte sectors (8 doubles) of the pivot row: only these columns of the other rows change; rows with a non-zero multiplier.  Both as ordered
    // (ascending, deterministic) LDS lists
    const int nsec = (n + SOL_SEC) / SOL_SEC;
    int nact = 0, nrows = 0;
#ifdef MLD_PIVOT_PROF
    long long tq2;
#endif
    if (!(LEG && (w.dbg & MLD_DBG_PIVOT_SYNC_R5)) && nsec <= SOL_NT && m <= LIST_NCH * SOL_NT) {      // one exchange for all chunks (list_counts)
        const unsigned long long before = (1ull << lane) - 1ull;
        bool act = false;
        if (tid < nsec) {
#pragma unroll
            for (int e = 0; e < SOL_SEC; ++e) { const int k = tid * SOL_SEC + e; if (k <= n && rowr[k] != 0.0) act = true; }
        }
        const unsigned long long bs = __ballot(act);
        if (lane == 0) sh.lcnt[0][wave] = __popcll(bs);
        unsigned long long br[LIST_NCH];
#pragma unroll
        for (int k = 0; k < LIST_NCH; ++k) {
            br[k] = 0ull;
            if (k * SOL_NT < m) {
                const int i = k * SOL_NT + tid;
                br[k] = __ballot(i < m && i != r && colc[i] != 0.0);
                if (lane == 0) sh.lcnt[1 + k][wave] = __popcll(br[k]);
            }
        }
        __syncthreads();
#ifdef MLD_PIVOT_PROF
        tq2 = wall_clock64();      // (on this path [1] is the flags and the exchange, [2] the scatter of both lists)
#endif
        int off, tot;
        list_counts(sh, 0, wave, off, tot);
        if (act) seclist[off + __popcll(bs & before)] = (unsigned short)tid;
        nact = tot;
#pragma unroll
        for (int k = 0; k < LIST_NCH; ++k) {
            if (k * SOL_NT < m) {
                list_counts(sh, 1 + k, wave, off, tot);
                if ((br[k] >> lane) & 1ull) rowlist[nrows + off + __popcll(br[k] & before)] = (unsigned short)(k * SOL_NT + tid);
                nrows += tot;
            }
        }
    } else {
        for (int t0 = 0; t0 < nsec; t0 += SOL_NT) {       // ordered compaction, SOL_NT sectors at a time
            const int t = t0 + tid;
            bool act = false;
            if (t < nsec) {
#pragma unroll
                for (int e = 0; e < SOL_SEC; ++e) { const int k = t * SOL_SEC + e; if (k <= n && rowr[k] != 0.0) act = true; }
            }
            nact = block_compact(sh, act, (unsigned short)t, w.seclist, nact);
        }
#ifdef MLD_PIVOT_PROF
        tq2 = wall_clock64();
#endif
        for (int i0 = 0; i0 < m; i0 += SOL_NT) {
            const int i = i0 + tid;
            nrows = block_compact(sh, i < m && i != r && colc[i] != 0.0, (unsigned short)i, w.rowlist, nrows);
        }
    }
    __syncthreads();
#ifdef MLD_PIVOT_PROF
    const long long tq3 = wall_clock64();
#endif
#ifdef MLD_ASSERT
    MLD_CHECK(w, nact <= (n + SOL_SEC) / SOL_SEC && nrows < m, 102, nact, nrows);
    for (int t = tid; t < nrows; t += SOL_NT) MLD_CHECK(w, (int)rowlist[t] < m, 103, t, rowlist[t]);
    for (int t = tid; t < nact; t += SOL_NT) MLD_CHECK(w, (int)seclist[t] < (n + SOL_SEC) / SOL_SEC, 104, t, seclist[t]);
#endif
    {
        const int ngrp = (nact + SOL_SPW - 1) / SOL_SPW;
        if (MLD_UPDATE_LEGACY_ALWAYS || (LEG && (w.dbg & MLD_DBG_UPDATE_R7))) {      // the update as it was (legacy instantiation)
            for (int g0 = 0; g0 < ngrp; g0 += 4) {
                switch (ngrp - g0) {
                case 1: s_update_rows<1>(D, ld, rowr, colc, rowlist, seclist, nrows, nact, g0, c, wave, lane); break;
                case 2: s_update_rows<2>(D, ld, rowr, colc, rowlist, seclist, nrows, nact, g0, c, wave, lane); break;
                case 3: s_update_rows<3>(D, ld, rowr, colc, rowlist, seclist, nrows, nact, g0, c, wave, lane); break;
                default: s_update_rows<4>(D, ld, rowr, colc, rowlist, seclist, nrows, nact, g0, c, wave, lane); break;
                }
            }
        } else {
            for (int g0 = 0; g0 < ngrp; g0 += 4) {
                switch (ngrp - g0) {
                case 1: s_update_rows_r7<1>(D, ld, rowr, colc, rowlist, seclist, nrows, nact, g0, c, wave, lane); break;
                case 2: s_update_rows_r7<2>(D, ld, rowr, colc, rowlist, seclist, nrows, nact, g0, c, wave, lane); break;
                case 3: s_update_rows_r7<3>(D, ld, rowr, colc, rowlist, seclist, nrows, nact, g0, c, wave, lane); break;
                default: s_update_rows_r7<4>(D, ld, rowr, colc, rowlist, seclist, nrows, nact, g0, c, wave, lane); break;
                }
            }
        }
    }
    if (tid == 0) {
        sh.rows += (unsigned long long)nrows * (unsigned long long)nact;   // 64-byte sectors updated
        sh.prof[0] += wall_clock64() - tp0;
#ifdef MLD_PIVOT_PROF
        sh.pprof[0] += tq1 - tp0; sh.pprof[1] += tq2 - tq1; sh.pprof[2] += tq3 - tq2; sh.pprof[3] += wall_clock64() - tq3;      // ([0]: with a look-ahead that declined, if any)
        sh.pcnt[0]++;
#endif
    }
    __syncthreads();
}

// the rank-1 update: entering column c, leaving row r, leaving variable goes to leave_value
template <bool L, bool LEG>
__device__ __forceinline__ void s_pivot_inl(const Ws &w, Shared &sh, int r, int c, double leave_value)
{
    const long long tp0 = wall_clock64();
    s_pivot_head<L, false, LEG>(w, sh, r, c, leave_value, (lds_f64 *)w.rowr, (lds_f64 *)w.colc, -1, -1);
    s_pivot_update<LEG>(w, sh, r, c, tp0);
}

// out-of-line copy for the cold callers (refactor, primal simplex): it keeps every selectable variant (MLD_DBG_PIVOT_SYNC_R5, MLD_DBG_UPDATE_R7)
__device__ __noinline__ void s_pivot(const Ws &w, Shared &sh, int r, int c, double leave_value) { s_pivot_inl<false, true>(w, sh, r, c, leave_value); }

// structural values (scaled space) into w.tmpx
__device__ void s_gather_x(const Ws &w, Shared &sh, double *x)
{
    __syncthreads();
    for (int c = threadIdx.x; c < w.n; c += SOL_NT) { const int j = w.nonbasic[c]; if (j < w.n) x[j] = w.xN[c]; }
    for (int r = threadIdx.x; r < sh.m; r += SOL_NT) { const int j = w.basic[r]; if (j < w.n) x[j] = w.xB[r]; }
    __syncthreads();
}

// largest |h - Gx - slack| over all rows (original data vs dictionary)
__device__ __noinline__ double s_check_residual(const Ws &w, Shared &sh)
{
    const int n = w.n, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = sh.m;
    lds_f64 *xs = (lds_f64 *)w.dabuf;
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += SOL_NT) { const int j = w.nonbasic[c]; if (j < n) xs[j] = w.xN[c]; }
    for (int r = threadIdx.x; r < m; r += SOL_NT) { const int j = w.basic[r]; if (j < n) xs[j] = w.xB[r]; }
    __syncthreads();
    double worst = 0.0;
    const int nl = live_count(w, sh);
    (void)m;
    int t_first = 0;
    if (w.csr_ptr) {
        // the original rows from their sparse copy, a thread per live row (round 4: 11 entries on average instead of a dense row of n: the check was 7.5 % of
        // the kernel once the presolve had halved the pivots); the cut rows below stay dense
        t_first = sh.nlive;
        for (int t = threadIdx.x; t < sh.nlive; t += SOL_NT) {
            const int i = w.live[t];
            double acc = 0.0;
            const int e1 = w.csr_ptr[i + 1];
            if (w.dbg & MLD_DBG_WALKS_SERIAL) { for (int e = w.csr_ptr[i]; e < e1; ++e) acc += w.csr_val[e] * xs[w.csr_col[e]]; }
            else {
                glb_cu16 *rc = (glb_cu16 *)w.csr_col; glb_cf64 *rv = (glb_cf64 *)w.csr_val;
                for (int e = w.csr_ptr[i]; e < e1; e += WALK_GROUP) {
                    int cj[WALK_GROUP]; double cg[WALK_GROUP], xv[WALK_GROUP];
#pragma unroll
                    for (int q = 0; q < WALK_GROUP; ++q) { const int eq = min(e + q, e1 - 1); cj[q] = rc[eq]; cg[q] = rv[eq]; }      // (past the end: the last entry again, not used)
#pragma unroll
                    for (int q = 0; q < WALK_GROUP; ++q) xv[q] = xs[cj[q]];
#pragma unroll
                    for (int q = 0; q < WALK_GROUP; ++q) if (e + q < e1) acc += cg[q] * xv[q];
                }
            }
            const int wh = w.where[n + i];
            MLD_CHECK(w, wh < n && -1 - wh < m, 136, i, wh);
            const double v = wh >= 0 ? w.xN[wh] : w.xB[-1 - wh];
            worst = fmax(worst, fabs(w.hs[i] - acc - v));
        }
    }
    for (int t0 = t_first + wave * 4; t0 < nl; t0 += SOL_NW * 4) {
        const glb_f64 *rp[4]; int ri[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { ri[q] = live_row(w, sh, t0 + q < nl ? t0 + q : t0); rp[q] = (const glb_f64 *)orig_row(w, ri[q]); }
        double s[4];
        wave_rows_dot4(rp[0], rp[1], rp[2], rp[3], xs, n, lane, s, (w.dbg & MLD_DBG_WALKS_SERIAL) != 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double t = wave_sum(s[q]);
            const int i = ri[q];
            if (lane == 0 && t0 + q < nl && !(w.skip[i] & 2)) {      // (a cut row that is no longer maintained has no slack value)
                const int wh = w.where[n + i];
                MLD_CHECK(w, wh < n && -1 - wh < m, 136, i, wh);
                const double v = wh >= 0 ? w.xN[wh] : w.xB[-1 - wh];
                worst = fmax(worst, fabs(orig_rhs(w, i) - t - v));
            }
        }
    }
    return block_max(sh, worst);
}

// rebuild the dictionary for the current basis from the original rows (complete pivoting)
// every non-basic column to the bound that makes its reduced cost dual feasible (free variables are boxed at +-S_BIG
// only when they have to rest there); the caller refreshes x_B afterwards
__device__ void s_place_all(const Ws &w)
{
    const int n = w.n;
    const double *d = w.dcost;
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += SOL_NT) {
        const int j = w.nonbasic[c];
        const double dc = d[c];
        double lo = w.lo[j], hi = w.hi[j];
        if (lo == hi) { w.at_upper[c] = 0; w.xN[c] = lo; }
        else if (dc >= 0) { if (lo == -S_INF) { lo = -S_BIG; w.lo[j] = lo; } w.at_upper[c] = 0; w.xN[c] = lo; }
        else { if (hi == S_INF) { hi = S_BIG; w.hi[j] = hi; } w.at_upper[c] = 1; w.xN[c] = hi; }
    }
    __syncthreads();
}

__device__ __noinline__ void s_refactor(const Ws &w, Shared &sh)      // (out of line: no plain pivot runs it)
{
    const int n = w.n, m = sh.m, ld = w.ld, tid = threadIdx.x;
    __syncthreads();
    // remember the non-basic state per variable id in g (value) / key (flag bits): reuse tmp arrays sized >= ntot? no:
    // values of structurals -> xo (n), at_upper of structurals -> tmpx (n); slacks are non-basic at 0 / lower.
    // want-basic flag of structural j -> ax[j]; row-free flag of row i -> key[i]
    for (int j = tid; j < n; j += SOL_NT) { w.ax[j] = 0.0; }
    for (int i = tid; i < m; i += SOL_NT) w.key[i] = 0.0;
    __syncthreads();
    for (int r = tid; r < m; r += SOL_NT) { const int j = w.basic[r]; if (j < n) w.ax[j] = 1.0; }
    for (int c = tid; c < n; c += SOL_NT) {
        const int j = w.nonbasic[c];
        if (j < n) { w.xo[j] = w.xN[c]; w.tmpx[j] = w.at_upper[c] ? 1.0 : 0.0; }
        else w.key[j - n] = 1.0;
    }
    __syncthreads();
    int nwant = 0;
    {
        double cnt = 0.0;
        for (int j = tid; j < n; j += SOL_NT) cnt += w.ax[j];
        nwant = (int)(block_sum(sh, cnt) + 0.5);
    }
    s_reset_dictionary(w, sh);
    for (int c = tid; c < n; c += SOL_NT) w.xN[c] = 0.0;
    for (int r = tid; r < m; r += SOL_NT) w.xB[r] = 0.0;
    __syncthreads();
    const int saved_p = sh.pivots, saved_c = sh.since_check;
    for (int k = 0; k < nwant; ++k) {
        // complete pivoting over (free rows) x (wanted columns still non-basic at their own index)
        double best = -1.0; int bidx = -1;
        const int wave = tid >> 6, lane = tid & 63;
        for (int r = wave; r < m; r += SOL_NW) {
            if (w.key[r] == 0.0) continue;
            const double *row = w.D + (size_t)r * ld;
            for (int c = lane; c < n; c += 64) {
                const int j = w.nonbasic[c];
                if (j < n && w.ax[j] != 0.0) { const double a = fabs(row[c]); if (a > best) { best = a; bidx = r * n + c; } }
            }
        }
        double bv;
        const int id = block_argmax(sh, best, bidx, &bv);
        if (id < 0 || !(bv > 0.0)) break;
        const int r = id / n, c = id - r * n;
        MLD_CHECK(w, r >= 0 && r < m && c >= 0 && c < n, 134, id, r);
        const int jc = w.nonbasic[c];
        s_pivot(w, sh, r, c, 0.0);
        if (tid == 0) { w.key[r] = 0.0; w.ax[jc] = 0.0; }
        __syncthreads();
    }
    if (tid == 0) { sh.pivots = saved_p; sh.since_check = saved_c; sh.refactors++; sh.perturbed = 0; }   // (the rebuilt dictionary has the true cost row)
    __syncthreads();
    for (int c = tid; c < n; c += SOL_NT) {
        const int j = w.nonbasic[c];
        if (j >= n) { w.xN[c] = 0.0; w.at_upper[c] = 0; }
        else if (w.ax[j] == 0.0) { w.xN[c] = w.xo[j]; w.at_upper[c] = w.tmpx[j] != 0.0; }
        else {   // a wanted variable that could not be pivoted in (numerically singular basis): park it at a bound
            const double dc = w.dcost[c];
            double lo = w.lo[j], hi = w.hi[j];
            if (lo == hi) { w.at_upper[c] = 0; w.xN[c] = lo; }
            else if (dc >= 0) { if (lo == -S_INF) { lo = -S_BIG; w.lo[j] = lo; } w.at_upper[c] = 0; w.xN[c] = lo; }
            else { if (hi == S_INF) { hi = S_BIG; w.hi[j] = hi; } w.at_upper[c] = 1; w.xN[c] = hi; }
        }
    }
    // If a wanted variable could not be pivoted in, the basis is another one and reduced costs may have the wrong sign:
    // boxed structurals move to the matching bound; a slack (or free) column cannot -- then the dictionary is restarted
    // from the slack basis with every column at its dual-feasible bound (the dual simplex re-solves from there).
    {
        __syncthreads();
        const double *dd = w.dcost;
        double bad = 0.0;
        for (int c = tid; c < n; c += SOL_NT) {
            const int j = w.nonbasic[c];
            double lo = w.lo[j], hi = w.hi[j];
            if (lo == hi) continue;
            const double dc = dd[c];
            const double viol = w.at_upper[c] ? dc : -dc;
            if (viol <= 1e-7) continue;
            if (j < n) {
                if (dc >= 0) { if (lo == -S_INF) { lo = -S_BIG; w.lo[j] = lo; } w.at_upper[c] = 0; w.xN[c] = lo; }
                else { if (hi == S_INF) { hi = S_BIG; w.hi[j] = hi; } w.at_upper[c] = 1; w.xN[c] = hi; }
            } else bad = 1.0;
        }
        if (block_max(sh, bad) > 0.0) {
            s_reset_dictionary(w, sh);
            s_place_all(w);
        }
    }
    for (int i = threadIdx.x; i < w.mcap; i += SOL_NT) w.dw[i] = 1.0;     // the rebuilt basis is the new devex reference framework
    s_refresh(w, sh);
}

// bounded dual simplex with Harris ratio test and Bland fallback; all threads return the same status
template <bool L, bool R6, bool LEG> __device__ __noinline__ int s_dual_simplex_impl(const Ws &w, Shared &sh, double cutoff, int max_pivots);
// (R6 = MLD_DBG_SELECT_R6: the loop with its earlier selection is an instantiation of its own, so that neither carries the other's instructions.
// LEG: the legacy instantiations, taken whenever MLD_DBG_PIVOT_SYNC_R5, MLD_DBG_SELECT_R6 or MLD_DBG_UPDATE_R7 is set, hold the earlier barriers, lists and
// row updates and choose among them at run time; the default one holds none of them -- the loop carries only the text it runs.)
#define MLD_DBG_LEGACY_LOOP (MLD_DBG_PIVOT_SYNC_R5 | MLD_DBG_SELECT_R6 | MLD_DBG_UPDATE_R7)
__device__ __forceinline__ int s_dual_simplex_pick(const Ws &w, Shared &sh, double cutoff, int max_pivots)
{
    if (w.dbg & MLD_DBG_SELECT_R6) return w.all_lds ? s_dual_simplex_impl<true, true, true>(w, sh, cutoff, max_pivots) : s_dual_simplex_impl<false, true, true>(w, sh, cutoff, max_pivots);
    if (w.dbg & MLD_DBG_LEGACY_LOOP) return w.all_lds ? s_dual_simplex_impl<true, false, true>(w, sh, cutoff, max_pivots) : s_dual_simplex_impl<false, false, true>(w, sh, cutoff, max_pivots);
    return w.all_lds ? s_dual_simplex_impl<true, false, false>(w, sh, cutoff, max_pivots) : s_dual_simplex_impl<false, false, false>(w, sh, cutoff, max_pivots);
}
__device__ int s_dual_simplex(const Ws &w, Shared &sh, double cutoff, int max_pivots)
{
    const long long t0 = wall_clock64();
    const long long p0 = sh.prof[0] + sh.prof[5];
    // One re-solve that needs more pivots than four times the size of the problem is cycling (Harris tolerances void Bland's guarantee; seen once in
    // ~300 000 bench instances: 29 167 pivots in one root re-solve, 2 s for the whole step): the dictionary is rebuilt from the original rows and
    // the solve gets one more allowance; after that the instance ends with what it has (LP_ITERLIMIT, as at the global pivot limit).
    const int lp_cap = 4 * (w.m0 + w.n) + 1000;
    int st = s_dual_simplex_pick(w, sh, cutoff, min(max_pivots, sh.pivots + lp_cap));
    __syncthreads();
    if (st == LP_ITERLIMIT && sh.pivots < max_pivots && !(sh.deadline && sh.timed_out)) {      // (not when the TimeLimit ended it: nothing is cycling)
        __syncthreads();
        s_refactor(w, sh);
        __syncthreads();
        st = s_dual_simplex_pick(w, sh, cutoff, min(max_pivots, sh.pivots + lp_cap));
    }
    __syncthreads();
    if (threadIdx.x == 0) sh.prof[1] += (wall_clock64() - t0) - (sh.prof[0] + sh.prof[5] - p0);
    __syncthreads();
    return st;
}
__device__ void s_reprice(const Ws &w, Shared &sh, const double *cost);
__device__ int s_primal_simplex(const Ws &w, Shared &sh, int max_pivots);

// Anti-stalling cost perturbation (oracle: perturb_costs / unperturb; Koberstein 2005, section 6.2): when a solve stalls (root LP, cut rounds,
// leaves, dives, node re-solves on dual degenerate instances -- heating is free while PV exports), every non-basic reduced cost is
// pushed away from zero in its feasible direction by a deterministic pseudo-random amount of relative size 1e-6..2e-6: the ties of the dual
// ratio test are broken and the solve no longer falls back on Bland's rule (measured on the CPU restatement, 2048 bench instances: 7.3 % of all
// pivots were Bland pivots, one cut round of one instance took 2 200 of them; 0.4 % with the perturbation).  When the perturbed problem is
// optimal the true cost row is restored (s_reprice) and, if some reduced cost then has the wrong sign, the bounded primal simplex finishes
// from this primal-feasible basis.
__device__ __noinline__ void s_perturb_costs(const Ws &w, Shared &sh)      // (out of line: once per solve at most)
{
    const int n = w.n;
    double *d = w.dcost;
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += SOL_NT) {
        const int j = w.nonbasic[c];
        if (w.lo[j] == w.hi[j]) continue;
        const unsigned hsh = (unsigned)j * 2654435761u;
        const double u = (double)(hsh >> 8) * (1.0 / 16777216.0);      // [0, 1) from the variable's id: the same in every slot and launch
        const double dc = d[c];
        const double eps = S_PERT * (1.0 + u) * (1.0 + fabs(dc));
        d[c] = dc + (w.at_upper[c] ? -eps : eps);
    }
    if (threadIdx.x == 0) sh.perturbed = 1;
    __syncthreads();
}

__device__ __noinline__ int s_unperturb(const Ws &w, Shared &sh, int st, int max_pivots)      // (out of line: the loop's five ways out)
{
    __syncthreads();
    if (!sh.perturbed) return st;
    __syncthreads();
    s_reprice(w, sh, w.qs);
    if (threadIdx.x == 0) sh.perturbed = 0;
    __syncthreads();
    if (st != LP_OPTIMAL) return st;
    const double *d = w.dcost;
    double bad = 0.0;
    for (int c = threadIdx.x; c < w.n; c += SOL_NT) {
        const int j = w.nonbasic[c];
        if (w.lo[j] == w.hi[j]) continue;
        if ((w.at_upper[c] ? d[c] : -d[c]) > S_DTOL) bad = 1.0;
    }
    if (!(block_max(sh, bad) > 0.0)) return LP_OPTIMAL;
    const int ps = s_primal_simplex(w, sh, max_pivots);
    __syncthreads();
    return ps == LP_OPTIMAL ? LP_OPTIMAL : LP_ITERLIMIT;
}

// The NEXT iteration's choice of s_dual_simplex_impl, made before the rows' update of the pivot (r1, c1) whose first half has just run: devex pricing on the x_B,
// weights, bounds and maps that pivot left behind, then the Harris ratio test on row r2 as the pending update will leave it -- D[r2, k] - colc1[r2] * rowr1[k]
// through s_upd on the first row's active sectors, the old entry of column c1 counting as 0, exactly as s_update_rows does it; the scaled first row itself if
// r2 == r1.  The raw row goes to w.rowr2 (k <= n), the eligible |a| to w.colc2, the clamped reduced costs to w.dabuf.  True (with r2, c2 and the leaving variable's
// target) when that iteration is a plain pivot; false when it does anything else (optimal, cut off, no eligible entry, a row to skip): the caller then finishes the
// first pivot alone and the loop makes that iteration as ever.  Only scratch is written.  Every thread returns the same.
template <bool L, bool R6>
__device__ __forceinline__ bool s_look_ahead(const Ws &w, Shared &sh, int r1, int c1, double cur, double cutoff, int &par, int &r2, int &c2, double &lv2)
{
    HOT_VIEW(L, w);
    const int n = w.n, ld = w.ld, m = sh.m, tid = threadIdx.x;
    constexpr bool r6 = R6;      // the selection as it was (s_dual_simplex_impl)
    SEL_CLOCK_START(ts);
    double myv = -S_INF; int myi = -1;
    for (int i = tid; i < m; i += SOL_NT) {
        if (h_skip[i]) continue;
        const int j = h_basic[i];
        const double v = fmax(h_lo[j] - h_xB[i], h_xB[i] - h_hi[j]);
        if (v > S_PTOL) {
            const double sc = v * v / h_dw[i];
            if (sc > myv) { myv = sc; myi = i; }
        }
    }
    double worst;
    const int r = sel_argmax1(sh, myv, myi, &worst, par, r6);      // (a thread without a candidate: -inf against a score > 0)
    SEL_CLOCK(sh, 5, ts);
    if (r < 0) return false;
    if (cur >= cutoff && !sh.perturbed) return false;
    MLD_CHECK(w, r < m, 105, r, 2);
    const int jr = h_basic[r];
    const double vlo = h_lo[jr] - h_xB[r], vhi = h_xB[r] - h_hi[jr];
    const bool below = vlo > vhi;
    const double viol = below ? vlo : vhi;
    const glb_f64 *row = (const glb_f64 *)(w.D + (size_t)r * ld);
    const lds_f64 *rowr1 = (const lds_f64 *)w.rowr, *colc1 = (const lds_f64 *)w.colc;
    const lds_u8 *sf = (const lds_u8 *)w.secflag;
    lds_f64 *raw = (lds_f64 *)w.rowr2, *ea = (lds_f64 *)w.colc2, *dal = (lds_f64 *)w.dabuf;
    const bool same = r == r1;
    const double mu = colc1[r];
    double emax = 0.0;
    for (int c0 = 0; c0 <= n; c0 += 4 * SOL_NT) {
        double av[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int c = c0 + q * SOL_NT + tid; av[q] = (c <= n && !same) ? row[c] : 0.0; }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = c0 + q * SOL_NT + tid;
            if (c > n) continue;
            double a;
            if (same) a = rowr1[c];
            else {
                a = av[q];
                if (mu != 0.0 && (sf[c / SOL_SEC] & 1)) a = s_upd(c == c1 ? 0.0 : a, mu, rowr1[c]);
            }
            raw[c] = a;
            if (c == n) continue;
            const int j = h_nonbasic[c];
            MLD_CHECK(w, j >= 0 && j < n + w.mcap, 111, c, j);
            const bool up = h_up[c];
            // (a > 0 is wanted when the row is below its bound and the column at its upper one, or neither; a < 0 otherwise: one compare of +-a, no nested branches)
            const bool el = r6 ? (h_lo[j] != h_hi[j]) && (below ? (up ? a > 0 : a < 0) : (up ? a < 0 : a > 0))
                               : (bool)((h_lo[j] != h_hi[j]) & ((below == up ? a : -a) > 0.0));
            const double aa = el ? fabs(a) : 0.0;
            const double dv = h_d[c];
            const double dc = fmax(up ? -dv : dv, 0.0);
            ea[c] = aa;
            dal[c] = dc;
            emax = fmax(emax, aa);
        }
    }
    emax = sel_max1(sh, emax, par, r6);      // (|a| or +0.0: no -0.0)
    SEL_CLOCK(sh, 6, ts);
    const double ptol = fmax(S_PIV_ABS, S_PIV_REL * emax);
    double tmax = S_INF;
    for (int c = tid; c < n; c += SOL_NT) {
        const double aa = ea[c];
        if (aa <= ptol) continue;
        tmax = fmin(tmax, (dal[c] + S_DTOL) / aa);
    }
    tmax = sel_min1(sh, tmax, par, r6);      // (the negated ratios are < 0, or -inf)
    SEL_CLOCK(sh, 7, ts);
    if (tmax == S_INF) return false;
    double bv = -1.0; int bi = -1;
    for (int c = tid; c < n; c += SOL_NT) {
        const double aa = ea[c];
        if (aa <= ptol) continue;
        if (dal[c] / aa <= tmax && aa > bv) { bv = aa; bi = c; }
    }
    double tmp;
    const int cbest = sel_argmax1(sh, bv, bi, &tmp, par, r6);      // (a thread without a candidate: -1.0 against |a| > ptol > 0)
    SEL_CLOCK(sh, 8, ts);
    if (cbest < 0) return false;
    MLD_CHECK(w, cbest < n, 106, cbest, 2);
    if (ea[cbest] < S_PIV_TINY && viol <= S_PTOL_SKIP) return false;
    r2 = r; c2 = cbest; lv2 = below ? h_lo[jr] : h_hi[jr];
    return true;
}

// A pivot of s_dual_simplex_impl and, when it is a plain one (try_pair: devex pricing, Harris ratio test; all hot arrays in LDS) and the loop's next iteration is one too, that pivot with it:
// two consecutive dual pivots of a dive or a re-solve repair the same few horizon steps, so most (row, sector) pairs of the second update are pairs of the first.
// After the first pivot's first half the next iteration is made on what it left in LDS (s_look_ahead), the second pivot's first half runs on corrected entries
// (s_pivot_head<L, true>), and ONE pass over the union of the two updates applies both in order (s_update_rows2): a shared pair is read and written once.  Nothing is
// left pending: on return the dictionary is fully updated.  Whatever the loop would do between the two pivots besides counting a stall -- a limit, the deadline, a
// verification, the perturbation, Bland's rule -- means no pair: the first pivot is finished alone (s_pivot_update) and the loop goes on unchanged.  cur, stall and
// last_obj leave as two iterations would leave them.
template <bool LEG> __device__ __forceinline__ void s_pair_update(const Ws &w, Shared &sh, int r1, int c1, int r2, int c2, long long tp0);
template <bool L, bool R6, bool LEG>
__device__ __forceinline__ void s_pivot_pair(const Ws &w, Shared &sh, int r1, int c1, double lv1, bool try_pair, double cutoff, int max_pivots, double &cur,
                                             int &stall, double &last_obj, int &par)
{
    const long long tp0 = wall_clock64();
    const int n = w.n, tid = threadIdx.x;
    const int nsec = (n + SOL_SEC) / SOL_SEC;
    lds_f64 *rowr = (lds_f64 *)w.rowr, *colc = (lds_f64 *)w.colc, *rowr2 = (lds_f64 *)w.rowr2, *colc2 = (lds_f64 *)w.colc2;
    lds_u8 *secflag = (lds_u8 *)w.secflag;
    s_pivot_head<L, false, LEG>(w, sh, r1, c1, lv1, rowr, colc, -1, -1);
    cur += sh.s_d[0];
    // the top of the loop's next iteration
    const int piv = sh.pivots;
    bool go = try_pair && piv < max_pivots && !(sh.deadline && (piv & 127) == 127) && sh.since_check < 512;
    int stall2 = stall; double last2 = last_obj;
    if (cur > last2 + 1e-12 * fmax(1.0, fabs(cur))) { stall2 = 0; last2 = cur; } else stall2++;
    go = go && stall2 <= 30;
    int r2 = -1, c2 = -1; double lv2 = 0.0;
    if (go) {
        for (int t = tid; t < nsec; t += SOL_NT) {      // active sectors of the first pivot's row (s_look_ahead's first barrier comes before its first use)
            bool act = false;
#pragma unroll
            for (int e = 0; e < SOL_SEC; ++e) { const int k = t * SOL_SEC + e; if (k <= n && rowr[k] != 0.0) act = true; }
            secflag[t] = act ? 1 : 0;
        }
        go = s_look_ahead<L, R6>(w, sh, r1, c1, cur, cutoff, par, r2, c2, lv2);
    }
    if (!go) { s_pivot_update<LEG>(w, sh, r1, c1, tp0); return; }
    stall = stall2; last_obj = last2;
    s_pivot_head<L, true, LEG>(w, sh, r2, c2, lv2, rowr2, colc2, r1, c1);
    cur += sh.s_d[0];
    s_pair_update<LEG>(w, sh, r1, c1, r2, c2, tp0);
}

// The one pass of a pair: both first halves have run -- rows r1 and r2 and their multiplier columns are staged in w.rowr / w.colc and w.rowr2 / w.colc2, and
// w.secflag bit 0 marks the first row's active sectors.  Builds the union lists and applies both updates in order (s_update_rows2_r7).
template <bool LEG>
__device__ __forceinline__ void s_pair_update(const Ws &w, Shared &sh, int r1, int c1, int r2, int c2, long long tp0)
{
    const int n = w.n, ld = w.ld, m = sh.m, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nsec = (n + SOL_SEC) / SOL_SEC;
    lds_f64 *rowr = (lds_f64 *)w.rowr, *colc = (lds_f64 *)w.colc, *rowr2 = (lds_f64 *)w.rowr2, *colc2 = (lds_f64 *)w.colc2;
    lds_u8 *secflag = (lds_u8 *)w.secflag;
#ifdef MLD_PIVOT_PROF
    const long long tq1 = wall_clock64();
    long long tq2;
#endif
    // union of the two rows' active sectors and of the two row sets (ordered); the counts of each set and of the overlaps (s1, s2, s12 sectors; n1, n2, n12 rows)
    int nact = 0, nrows = 0;
    unsigned long long s1, s2, s12, n1, n2, n12;
    if (!(LEG && (w.dbg & MLD_DBG_PIVOT_SYNC_R5)) && nsec <= SOL_NT && m <= LIST_NCH * SOL_NT) {      // one exchange for all chunks and all six counts (list_counts)
        const unsigned long long before = (1ull << lane) - 1ull;
        int f = 0;
        if (tid < nsec) {
            bool act = false;
#pragma unroll
            for (int e = 0; e < SOL_SEC; ++e) { const int k = tid * SOL_SEC + e; if (k <= n && rowr2[k] != 0.0) act = true; }
            f = (secflag[tid] & 1) | (act ? 2 : 0);
            secflag[tid] = (unsigned char)f;
        }
        const unsigned long long bs1 = __ballot((f & 1) != 0), bs2 = __ballot((f & 2) != 0);
        if (lane == 0) sh.lcnt[0][wave] = LIST_PACK(bs1, bs2);
        unsigned long long br[LIST_NCH];      // rows in either set
#pragma unroll
        for (int k = 0; k < LIST_NCH; ++k) {
            br[k] = 0ull;
            if (k * SOL_NT < m) {
                const int i = k * SOL_NT + tid;
                const bool in1 = i < m && i != r1 && i != r2 && colc[i] != 0.0, in2 = i < m && i != r2 && colc2[i] != 0.0;
                const unsigned long long b1 = __ballot(in1), b2 = __ballot(in2);
                br[k] = b1 | b2;
                if (lane == 0) sh.lcnt[1 + k][wave] = LIST_PACK(b1, b2);
            }
        }
        __syncthreads();
#ifdef MLD_PIVOT_PROF
        tq2 = wall_clock64();
#endif
        lds_u16 *seclist_w = (lds_u16 *)w.seclist2, *rowlist_w = (lds_u16 *)w.rowlist2;
        int off, tot;
        list_counts(sh, 0, wave, off, tot);
        if (f) seclist_w[LIST_UNION(off) + __popcll((bs1 | bs2) & before)] = (unsigned short)tid;
        s1 = tot & 1023; s2 = (tot >> 10) & 1023; s12 = tot >> 20;
        nact = LIST_UNION(tot);
        n1 = n2 = n12 = 0ull;
#pragma unroll
        for (int k = 0; k < LIST_NCH; ++k) {
            if (k * SOL_NT < m) {
                list_counts(sh, 1 + k, wave, off, tot);
                if ((br[k] >> lane) & 1ull) rowlist_w[nrows + LIST_UNION(off) + __popcll(br[k] & before)] = (unsigned short)(k * SOL_NT + tid);
                n1 += tot & 1023; n2 += (tot >> 10) & 1023; n12 += tot >> 20;
                nrows += LIST_UNION(tot);
            }
        }
    } else {      // chunk by chunk; the counts packed into one exact double per list
        double cnt_s = 0.0;
        for (int t0 = 0; t0 < nsec; t0 += SOL_NT) {
            const int t = t0 + tid;
            int f = 0;
            if (t < nsec) {
                bool act = false;
#pragma unroll
                for (int e = 0; e < SOL_SEC; ++e) { const int k = t * SOL_SEC + e; if (k <= n && rowr2[k] != 0.0) act = true; }
                f = (secflag[t] & 1) | (act ? 2 : 0);
                secflag[t] = (unsigned char)f;
            }
            cnt_s += (double)(f & 1) + 65536.0 * (double)(f >> 1) + 4294967296.0 * (double)(f == 3);
            nact = block_compact(sh, f != 0, (unsigned short)t, w.seclist2, nact);
        }
#ifdef MLD_PIVOT_PROF
        tq2 = wall_clock64();
#endif
        double cnt_r = 0.0;
        for (int i0 = 0; i0 < m; i0 += SOL_NT) {
            const int i = i0 + tid;
            const bool in1 = i < m && i != r1 && i != r2 && colc[i] != 0.0, in2 = i < m && i != r2 && colc2[i] != 0.0;
            cnt_r += (double)in1 + 65536.0 * (double)in2 + 4294967296.0 * (double)(in1 && in2);
            nrows = block_compact(sh, in1 || in2, (unsigned short)i, w.rowlist2, nrows);
        }
        cnt_s = block_sum(sh, cnt_s);
        cnt_r = block_sum(sh, cnt_r);
        const unsigned long long cs = (unsigned long long)cnt_s, cr = (unsigned long long)cnt_r;
        s1 = cs & 0xffffull; s2 = (cs >> 16) & 0xffffull; s12 = cs >> 32; n1 = cr & 0xffffull; n2 = (cr >> 16) & 0xffffull; n12 = cr >> 32;
    }
    __syncthreads();
#ifdef MLD_PIVOT_PROF
    const long long tq3 = wall_clock64();
#endif
    const lds_u16 *seclist = (const lds_u16 *)w.seclist2, *rowlist = (const lds_u16 *)w.rowlist2;
#ifdef MLD_ASSERT
    MLD_CHECK(w, nact <= nsec && nrows < m, 102, nact, nrows);
    for (int t = tid; t < nrows; t += SOL_NT) MLD_CHECK(w, (int)rowlist[t] < m && (int)rowlist[t] != r2, 103, t, rowlist[t]);
    for (int t = tid; t < nact; t += SOL_NT) MLD_CHECK(w, (int)seclist[t] < nsec, 104, t, seclist[t]);
#endif
    {
        glb_f64 *D = (glb_f64 *)w.D;
        const int ngrp = (nact + SOL_SPW - 1) / SOL_SPW;
        if (MLD_UPDATE_LEGACY_ALWAYS || (LEG && (w.dbg & MLD_DBG_UPDATE_R7))) {      // the update as it was (legacy instantiation)
            for (int g0 = 0; g0 < ngrp; g0 += 4) {
                switch (ngrp - g0) {
                case 1: s_update_rows2<1>(D, ld, rowr, colc, rowr2, colc2, rowlist, seclist, secflag, nrows, nact, g0, r1, c1, c2, wave, lane); break;
                case 2: s_update_rows2<2>(D, ld, rowr, colc, rowr2, colc2, rowlist, seclist, secflag, nrows, nact, g0, r1, c1, c2, wave, lane); break;
                case 3: s_update_rows2<3>(D, ld, rowr, colc, rowr2, colc2, rowlist, seclist, secflag, nrows, nact, g0, r1, c1, c2, wave, lane); break;
                default: s_update_rows2<4>(D, ld, rowr, colc, rowr2, colc2, rowlist, seclist, secflag, nrows, nact, g0, r1, c1, c2, wave, lane); break;
                }
            }
        } else {
            for (int g0 = 0; g0 < ngrp; g0 += 4) {
                switch (ngrp - g0) {
                case 1: s_update_rows2_r7<1>(D, ld, rowr, colc, rowr2, colc2, rowlist, seclist, secflag, nrows, nact, g0, r1, c1, c2, wave, lane); break;
                case 2: s_update_rows2_r7<2>(D, ld, rowr, colc, rowr2, colc2, rowlist, seclist, secflag, nrows, nact, g0, r1, c1, c2, wave, lane); break;
                case 3: s_update_rows2_r7<3>(D, ld, rowr, colc, rowr2, colc2, rowlist, seclist, secflag, nrows, nact, g0, r1, c1, c2, wave, lane); break;
                default: s_update_rows2_r7<4>(D, ld, rowr, colc, rowr2, colc2, rowlist, seclist, secflag, nrows, nact, g0, r1, c1, c2, wave, lane); break;
                }
            }
        }
    }
    if (tid == 0) {
        // 64-byte sectors moved: |R1 x S1| + |R2 x S2| - |(R1 and R2) x (S1 and S2)|
        sh.rows += n1 * s1 + n2 * s2 - n12 * s12;
        sh.prof[0] += wall_clock64() - tp0;
#ifdef MLD_PIVOT_PROF
        sh.pprof[4] += tq1 - tp0; sh.pprof[5] += tq2 - tq1; sh.pprof[6] += tq3 - tq2; sh.pprof[7] += wall_clock64() - tq3;      // ([4]: both first halves and the look-ahead)
        sh.pcnt[1]++;
#endif
    }
    __syncthreads();
}

// Blocks of the loop of s_dual_simplex_impl that a plain pivot does not run, out of line, so that the text a plain pivot fetches lies together.
// (1) The verification of the dictionary against the original rows, with a refactorisation if it has drifted past `tol` (four sites: every 512 pivots, at an
// optimum, before a cutoff is believed, before a small violation without an eligible entry is).  pre_barrier: every wave must have read sh.since_check before
// thread 0 resets it.  True when the dictionary was rebuilt (the skip marks are cleared; the caller recomputes the objective and starts the iteration again).
template <bool L>
__device__ __noinline__ bool s_loop_verify(const Ws &w, Shared &sh, double tol, bool pre_barrier, bool dbg_decides)
{
    HOT_VIEW(L, w);
    const int tid = threadIdx.x;
    const long long tr0 = wall_clock64();
    if (pre_barrier) __syncthreads();
    if (tid == 0) sh.since_check = 0;
    bool bad = s_check_residual(w, sh) > tol;
    if (dbg_decides) {
        if (w.dbg & MLD_DBG_REFACTOR_ALWAYS) bad = true;       // diagnostics: refactor at every check
        if (w.dbg & MLD_DBG_REFACTOR_NEVER) bad = false;      // diagnostics: never refactor
    }
    if (bad) s_refactor(w, sh);
    __syncthreads();
    if (tid == 0) sh.prof[5] += wall_clock64() - tr0;
    if (bad) for (int i = tid; i < w.mcap; i += SOL_NT) h_skip[i] &= 2;
    return bad;
}
// (2) The flips of the long-step ratio test: the columns marked by dal[c] == -2.0 move to their other bounds.  (The test's group loop stays in the loop: more
// than a third of the root LP's pivots go through it; flips are what few of them end in.)
template <bool L>
__device__ __noinline__ void s_loop_flips(const Ws &w, Shared &sh, int cbest, lds_f64 *ea, lds_f64 *dal)
{
    HOT_VIEW(L, w);
    const int n = w.n, ld = w.ld, m = sh.m, tid = threadIdx.x;
    // move the passed variables to their other bounds: x_B -= sum_f D[:, c_f] * (new - old), then the bookkeeping of the columns
    __syncthreads();
    if (tid == 0 && dal[cbest] == -2.0) dal[cbest] = 0.0;     // (the entering column itself is never flipped)
    __syncthreads();
    int nF = 0;
    for (int c0 = 0; c0 < n; c0 += SOL_NT) {
        const int c = c0 + tid;
        nF = block_compact(sh, c < n && dal[c] == -2.0, (unsigned short)c, w.seclist, nF);
    }
    __syncthreads();
    MLD_MARK(w, sh, 5000 + nF);
    MLD_CHECK(w, nF <= n && nF <= (int)(w.rowlist - w.seclist), 107, nF, cbest);
#ifdef MLD_ASSERT
    for (int f = tid; f < nF; f += SOL_NT) MLD_CHECK(w, (int)w.seclist[f] < n, 108, f, w.seclist[f]);
#endif
    lds_f64 *dlt = ea;                                        // step of each flipped column (the staged |a| are not needed any more: n + 2 doubles)
    for (int f = tid; f < nF; f += SOL_NT) {
        const int c = w.seclist[f], j = h_nonbasic[c];
        dlt[f] = (h_up[c] ? h_lo[j] : h_hi[j]) - h_xN[c];
    }
    __syncthreads();
    const glb_f64 *Dg = (const glb_f64 *)w.D;
    for (int i = tid; i < m; i += SOL_NT) {
        if (h_skip[i] & 2) continue;                          // rows that are not maintained
        double acc = 0.0;
        int f = 0;
        for (; f + 4 <= nF; f += 4) {
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = Dg[(size_t)i * ld + w.seclist[f + q]];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc += v[q] * dlt[f + q];
        }
        for (; f < nF; ++f) acc += Dg[(size_t)i * ld + w.seclist[f]] * dlt[f];
        h_xB[i] -= acc;
    }
    __syncthreads();
    for (int f = tid; f < nF; f += SOL_NT) {
        const int c = w.seclist[f], j = h_nonbasic[c];
        const bool up = h_up[c];
        h_xN[c] = up ? h_lo[j] : h_hi[j];
        h_up[c] = !up;
    }
    __syncthreads();
}

template <bool L, bool R6, bool LEG>
__device__ __noinline__ int s_dual_simplex_impl(const Ws &w, Shared &sh, double cutoff, int max_pivots)
{
    HOT_VIEW(L, w);
    const int n = w.n, ld = w.ld, tid = threadIdx.x;
    const int m = sh.m;
    bool pert_ok = !w.P && !(w.dbg & MLD_DBG_NO_PERTURB);      // one perturbation per solve (diagnostics: MLD_DBG_NO_PERTURB switches it off); while the cost row is
                                                 // perturbed the objective cutoff below is suspended -- the caller compares the true value after s_unperturb, only where no cutoff reads the (perturbed) objective
    for (int i = tid; i < w.mcap; i += SOL_NT) { h_skip[i] &= 2; h_dw[i] = 1.0; }   // bit 1 (row never binding, s_mark_dead) stays; new devex reference framework: this basis
    int stall = 0, par = 0;
    double last_obj = -S_INF, cur = 0.0;
    bool fresh_obj = true;                 // objective is recomputed at entry and after a refactor, tracked incrementally otherwise
    const double *d = w.dcost;
    // MLD_DBG_SELECT_R6: the selection as it was before its reductions left the LDS crossbar -- wave reductions through __shfl_down with a serial combine of
    // the waves' partials, the eligibility test of pass 1 as nested branches (DESIGN section 6).  The pricing scan, the loads of pass 1 and passes 2 and 3 of
    // the ratio test are the same in both.
    constexpr bool r6 = R6;
    for (;;) {
        SEL_CLOCK_START(ts);
        __syncthreads();
        if (sh.pivots >= max_pivots) return s_unperturb(w, sh, LP_ITERLIMIT, max_pivots);
        if (sh.deadline && (sh.pivots & 127) == 127) {      // TimeLimit inside one LP (ADVICE r3: a root LP or a leaf of thousands of pivots must not outlast it)
            if (tid == 0) sh.timed_out = wall_clock64() > sh.deadline ? 1 : 0;
            __syncthreads();
            const int to = sh.timed_out;
            __syncthreads();
            if (to) return s_unperturb(w, sh, LP_ITERLIMIT, max_pivots);
        }
        const int since = sh.since_check;
        if (since >= 512) {   // a long solve never reaches the verification at an optimum: verify on the way
            // Every wave must have READ sh.since_check before thread 0 resets it (round 4: this barrier was missing -- a wave that arrived late read 0,
            // skipped this block while the others ran its barriers, and the workgroup went on desynchronised: reductions over half-written buffers, a
            // leaving row of -1 or a stale column index used as a row.  The one write-after-read hazard on a shared scalar the audit of DESIGN section 4e
            // found; the other three resets below sit behind a barrier of their own.)
            if (s_loop_verify<L>(w, sh, S_RESID_TOL, true, false)) { fresh_obj = true; continue; }
        }
        if (fresh_obj) { cur = s_objective(w, sh); fresh_obj = false; }
        if (cur > last_obj + 1e-12 * fmax(1.0, fabs(cur))) { stall = 0; last_obj = cur; } else stall++;
        if (stall > 30 && pert_ok && !sh.perturbed) { pert_ok = false; s_perturb_costs(w, sh); stall = 0; last_obj = -S_INF; fresh_obj = true; continue; }
        const bool bland = stall > 30;
        // leaving row: dual devex pricing, largest violation^2 / weight (or smallest variable id while stalling)
        double myv = -S_INF; int myi = -1; int myid = 0x7fffffff, myrow = -1;
        SEL_CLOCK(sh, 0, ts);
        for (int i = tid; i < m; i += SOL_NT) {
            if (h_skip[i]) continue;
            const int j = h_basic[i];
            MLD_CHECK(w, j >= 0 && j < n + w.mcap, 110, i, j);
            const double v = fmax(h_lo[j] - h_xB[i], h_xB[i] - h_hi[j]);
            if (v > S_PTOL) {
                const double sc = v * v / h_dw[i];
                if (sc > myv) { myv = sc; myi = i; }
                if (j < myid) { myid = j; myrow = i; }
            }
        }
        double worst;
        int r = sel_argmax1(sh, myv, myi, &worst, par, r6);      // (a thread without a candidate: -inf against a score > 0)
        SEL_CLOCK(sh, 1, ts);
        if (r < 0) {

            if (since >= 64) {
                if (s_loop_verify<L>(w, sh, S_RESID_TOL, false, true)) { fresh_obj = true; continue; }      // (diagnostics: MLD_DBG_REFACTOR_ALWAYS / _NEVER decide here)
            }
            return s_unperturb(w, sh, LP_OPTIMAL, max_pivots);
        }
        if (bland) r = block_argmin_int(sh, myid, myrow);
        MLD_CHECK(w, r >= 0 && r < m, 105, r, bland);
        if (cur >= cutoff && !sh.perturbed) {
            // a cutoff is a claim about the bound: verify the dictionary first if it has moved since the last check
            if (since >= 64) {
                if (s_loop_verify<L>(w, sh, S_RESID_TOL, true, false)) { fresh_obj = true; continue; }
            }
            return LP_CUTOFF;
        }
        const int jr = h_basic[r];
        const double vlo = h_lo[jr] - h_xB[r], vhi = h_xB[r] - h_hi[jr];
        const bool below = vlo > vhi;
        const double viol = below ? vlo : vhi;
        const glb_f64 *row = (const glb_f64 *)(w.D + (size_t)r * ld);
        const glb_f64 *dg = (const glb_f64 *)d; const lds_f64 *dl = (const lds_f64 *)d;      // only the one that matches w.dc_lds is dereferenced
        const bool dlds = L || w.dc_lds;
        // one global pass: eligible |a_c| (0 when the column cannot enter) and the clamped reduced cost, staged in LDS
        lds_f64 *ea = (lds_f64 *)w.rowr, *dal = (lds_f64 *)w.dabuf;
        double emax = 0.0;
        for (int c0 = 0; c0 < n; c0 += 4 * SOL_NT) {      // the row and the cost row: all loads in flight before the first use
            double av[4], dv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int c = c0 + q * SOL_NT + tid; av[q] = c < n ? row[c] : 0.0; dv[q] = c < n ? (dlds ? dl[c] : dg[c]) : 0.0; }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + q * SOL_NT + tid;
                if (c >= n) continue;
                const int j = h_nonbasic[c];
                MLD_CHECK(w, j >= 0 && j < n + w.mcap, 111, c, j);
                const double a = av[q];
                const bool up = h_up[c];
                // (a > 0 is wanted when the row is below its bound and the column at its upper one, or neither; a < 0 otherwise: one compare of +-a, no nested branches)
                const bool el = r6 ? (h_lo[j] != h_hi[j]) && (below ? (up ? a > 0 : a < 0) : (up ? a < 0 : a > 0))
                                   : (bool)((h_lo[j] != h_hi[j]) & ((below == up ? a : -a) > 0.0));
                const double aa = el ? fabs(a) : 0.0;
                ea[c] = aa;
                dal[c] = fmax(up ? -dv[q] : dv[q], 0.0);
                emax = fmax(emax, aa);
            }
        }
        emax = sel_max1(sh, emax, par, r6);      // (|a| or +0.0: no -0.0)
        SEL_CLOCK(sh, 2, ts);
        const double ptol = fmax(S_PIV_ABS, S_PIV_REL * emax);
        // Harris bound on the step (tmax) and the exact minimum ratio (rmin)
        double tmax = S_INF, rmin = S_INF;
        for (int c = tid; c < n; c += SOL_NT) {
            const double aa = ea[c];
            if (aa <= ptol) continue;
            tmax = fmin(tmax, (dal[c] + S_DTOL) / aa);
            if (r6 || bland) rmin = fmin(rmin, dal[c] / aa);      // (read under Bland's rule only)
        }
        tmax = sel_min1(sh, tmax, par, r6);      // (the negated ratios are < 0, or -inf)
        SEL_CLOCK(sh, 3, ts);
        if (tmax == S_INF) {
            if (viol <= S_PTOL_SKIP) { __syncthreads(); if (tid == 0) h_skip[r] |= 1; continue; }
            if (since > 0 && viol <= 1e-3) {
                // a SMALL violation without an eligible entry may be accumulated error (a degenerate basic variable drifting
                // off its bound) rather than infeasibility: if the dictionary's discrepancy against the original rows is of
                // the violation's size, re-derive it before believing the row.
                if (s_loop_verify<L>(w, sh, 0.1 * viol, true, false)) { fresh_obj = true; continue; }
            }
            return s_unperturb(w, sh, LP_INFEASIBLE, max_pivots);
        }
        // entering column
        int cbest;
        bool long_step = false;
        if (bland) {
            rmin = block_min(sh, rmin);
            int key = 0x7fffffff, pay = -1;
            for (int c = tid; c < n; c += SOL_NT) {
                const double aa = ea[c];
                if (aa <= ptol) continue;
                const int j = h_nonbasic[c];
                if (dal[c] / aa <= rmin * (1 + 1e-12) + 1e-300 && j < key) { key = j; pay = c; }
            }
            cbest = block_argmin_int(sh, key, pay);
        } else if (sh.bfrt) {
            // Long-step ("bound flipping") ratio test for boxed variables (Fourer 1994; Maros 2003; oracle dual_simplex_impl): along the dual step the
            // objective rises with slope = the leaving row's violation; passing the breakpoint of a BOXED non-basic variable lowers the slope by
            // |a_rj| (hi_j - lo_j) and the variable simply moves to its other bound -- no pivot.  The breakpoints inside one Harris window are passed
            // together while the slope stays positive; the entering variable is the largest |a| of the first group that cannot be passed.
            // Switched on for the root LP only (k_solve): there a heating decision that ends at its upper bound costs two pivots without it.
            double slope = viol, tm = tmax, a_best = 0.0;
            int nflip_groups = 0;
            cbest = -1;
#ifdef MLD_PIVOT_PROF
            const long long tl0 = wall_clock64();
            int ngroups = 0;
#endif
            for (;;) {
#ifdef MLD_PIVOT_PROF
                ngroups++;
#endif
                double drop = 0.0, bv = -1.0; int bi = -1;
                for (int c = tid; c < n; c += SOL_NT) {
                    const double aa = ea[c];
                    if (aa <= ptol || !(dal[c] / aa <= tm)) continue;
                    const int j = h_nonbasic[c];
                    const double lo = h_lo[j], hi = h_hi[j];
                    drop += (lo > -0.5 * S_BIG && hi < 0.5 * S_BIG) ? aa * (hi - lo) : S_INF;
                    if (aa > bv) { bv = aa; bi = c; }
                }
                drop = block_sum(sh, drop);
                cbest = sel_argmax1(sh, bv, bi, &a_best, par, r6);      // (a thread without a candidate: -1.0 against |a| > ptol > 0)
                if (!(slope - drop > S_PTOL)) break;              // this group holds the entering variable
                slope -= drop;
                __syncthreads();
                for (int c = tid; c < n; c += SOL_NT) {           // the group is passed: its members flip (marked by a negative reduced cost) and leave the test
                    const double aa = ea[c];
                    if (aa <= ptol || !(dal[c] / aa <= tm)) continue;
                    dal[c] = -2.0;
                }
                __syncthreads();
                for (int c = tid; c < n; c += SOL_NT) if (dal[c] == -2.0) ea[c] = 0.0;
                __syncthreads();
                nflip_groups++;
                double t2 = S_INF;
                for (int c = tid; c < n; c += SOL_NT) { const double aa = ea[c]; if (aa > ptol) t2 = fmin(t2, (dal[c] + S_DTOL) / aa); }
                tm = sel_min1(sh, t2, par, r6);                   // (the negated ratios are < 0, or -inf)
                if (tm == S_INF) break;                           // every breakpoint passed: the last group's largest entry enters after all
            }
            if (cbest >= 0 && nflip_groups > 0) {
                s_loop_flips<L>(w, sh, cbest, ea, dal);      // (out of line: the passed variables move to their other bounds)
                fresh_obj = true;                                         // the flips moved the objective: recompute it at the next iteration
            }
#ifdef MLD_PIVOT_PROF
            if (tid == 0) { sh.pcnt[2] += wall_clock64() - tl0; sh.pcnt[3]++; sh.pcnt[4] += ngroups; sh.pcnt[5] += nflip_groups; sh.pcnt[6] += (cbest >= 0 && nflip_groups > 0); }
#endif
            if (cbest >= 0 && a_best < S_PIV_TINY && viol <= S_PTOL_SKIP && nflip_groups == 0) { __syncthreads(); if (tid == 0) h_skip[r] |= 1; continue; }
            if (cbest < 0) return s_unperturb(w, sh, LP_INFEASIBLE, max_pivots);
            MLD_CHECK(w, cbest < n, 106, cbest, 1);
            long_step = true;      // (the guards below are the other branches'; the pivot itself is the common one)
        } else {
            double bv = -1.0; int bi = -1;
            for (int c = tid; c < n; c += SOL_NT) {
                const double aa = ea[c];
                if (aa <= ptol) continue;
                if (dal[c] / aa <= tmax && aa > bv) { bv = aa; bi = c; }
            }
            double tmp;
            cbest = sel_argmax1(sh, bv, bi, &tmp, par, r6);      // (a thread without a candidate: -1.0 against |a| > ptol > 0)
            SEL_CLOCK(sh, 4, ts);
        }
        if (cbest < 0) return s_unperturb(w, sh, LP_INFEASIBLE, max_pivots);   // cannot happen (tmax finite), kept as a guard
        MLD_CHECK(w, cbest < n, 106, cbest, 0);
        if (!long_step && ea[cbest] < S_PIV_TINY && viol <= S_PTOL_SKIP) {
            // a violation within the skip tolerance whose only pivots are tiny: the dual step d_q / |a_q| would be huge and the
            // entries the ratio test ignored (|a| <= ptol) would carry it into their reduced costs -- dual feasibility, and with
            // it the bound, is lost (seen: violation 5e-8, pivot 1.7e-7, step 3e9).  The row counts as satisfied.
            __syncthreads(); if (tid == 0) h_skip[r] |= 1; continue;
        }
        // the pivot, and the next one with it where both are plain (devex pricing and Harris test: not under Bland's rule, not in the root LP's long-step test, not with
        // a quadratic cost) and the shape has the LDS for it
        s_pivot_pair<L, R6, LEG>(w, sh, r, cbest, below ? h_lo[jr] : h_hi[jr], L && w.pair && !bland && !long_step && !w.P, cutoff, max_pivots, cur, stall, last_obj, par);
    }
}


// ---- convex-QP relaxations: re-pricing, bounded primal simplex, simplicial decomposition -------------------------
#define LP_UNBOUNDED 4
#define SD_PMAX 32

// reduced costs of the current basis for the structural cost vector `cost` (slacks cost nothing)
__device__ void s_reprice(const Ws &w, Shared &sh, const double *cost)
{
    const int n = w.n, ld = w.ld, tid = threadIdx.x;
    double *d = w.dcost;
    __syncthreads();
    // compact the basic structural rows with a non-zero cost (ordered -> deterministic sums)
    int nr = 0;
    for (int r0 = 0; r0 < sh.m; r0 += SOL_NT) {
        const int r = r0 + tid;
        const bool f = r < sh.m && w.basic[r] < n && cost[w.basic[r]] != 0.0;
        nr = block_compact(sh, f, (unsigned short)r, w.rowlist, nr);
    }
    __syncthreads();
    MLD_CHECK(w, nr <= sh.m && sh.m <= w.mcap, 135, nr, sh.m);
    for (int t = tid; t < nr; t += SOL_NT) w.colc[t] = cost[w.basic[w.rowlist[t]]];
    __syncthreads();
    for (int c = tid; c <= n; c += SOL_NT) {
        double acc = 0.0;
        if (c < n) { const int j = w.nonbasic[c]; if (j < n) acc = cost[j]; }
        int t = 0;
        for (; t + 4 <= nr; t += 4) {
            const double v0 = w.D[(size_t)w.rowlist[t] * ld + c], v1 = w.D[(size_t)w.rowlist[t + 1] * ld + c],
                         v2 = w.D[(size_t)w.rowlist[t + 2] * ld + c], v3 = w.D[(size_t)w.rowlist[t + 3] * ld + c];
            if (c < n) { acc -= w.colc[t] * v0; acc -= w.colc[t + 1] * v1; acc -= w.colc[t + 2] * v2; acc -= w.colc[t + 3] * v3; }
            else { acc += w.colc[t] * v0; acc += w.colc[t + 1] * v1; acc += w.colc[t + 2] * v2; acc += w.colc[t + 3] * v3; }
        }
        for (; t < nr; ++t) { const double v0 = w.D[(size_t)w.rowlist[t] * ld + c]; if (c < n) acc -= w.colc[t] * v0; else acc += w.colc[t] * v0; }
        d[c] = acc;
    }
    __syncthreads();
}

// bounded primal simplex from a primal-feasible basis (Dantzig pricing, Harris ratio test, Bland while stalling)
__device__ int s_primal_simplex(const Ws &w, Shared &sh, int max_pivots)
{
    const int n = w.n, ld = w.ld, tid = threadIdx.x;
    const double *d = w.dcost;
    int stall = 0;
    double last_obj = S_INF;
    for (;;) {
        __syncthreads();
        const int m = sh.m;
        if (sh.pivots >= max_pivots) return LP_ITERLIMIT;
        const double cur = s_objective(w, sh);
        if (cur < last_obj - 1e-12 * fmax(1.0, fabs(cur))) { stall = 0; last_obj = cur; } else stall++;
        // cycling (round 4): Bland's rule on the entering side with Harris' ratio test is no guarantee, and this routine has no refactorisation of its own -- a QP
        // relaxation's return to the LP(q) vertex burnt 40 000 pivots (2 s) at one objective value on a dictionary grown to 1e13 after a pivot of 1e-6.  The caller
        // re-derives the dictionary and goes on with the LP bound of the node (s_sd_relax)
        if (stall > 2 * (n + m) + 500) return LP_ITERLIMIT;
        const bool bland = stall > 30;
        // entering column
        double bv = -S_INF; int bi = -1; int key = 0x7fffffff, pay = -1;
        for (int k = tid; k < n; k += SOL_NT) {
            const int j = w.nonbasic[k];
            if (w.lo[j] == w.hi[j]) continue;
            const double viol = w.at_upper[k] ? d[k] : -d[k];
            if (viol <= S_DTOL) continue;
            if (viol > bv) { bv = viol; bi = k; }
            if (j < key) { key = j; pay = k; }
        }
        double tmp;
        int c = block_argmax(sh, bv, bi, &tmp);
        if (c < 0) return LP_OPTIMAL;
        if (bland) c = block_argmin_int(sh, key, pay);
        const int jc = w.nonbasic[c];
        const double dir = w.at_upper[c] ? -1.0 : 1.0;
        // stage the column in LDS (colc) and find its largest magnitude
        double amax = 0.0;
        for (int i = tid; i < m; i += SOL_NT) { const double a = (w.skip[i] & 2) ? 0.0 : w.D[(size_t)i * ld + c] * dir; w.colc[i] = a; amax = fmax(amax, fabs(a)); }   // (rows that are not maintained take no part: linear-cost mode)
        amax = block_max(sh, amax);
        const double ptol = fmax(S_PIV_ABS, S_PIV_REL * amax);
        double tmax = w.hi[jc] - w.lo[jc];
        for (int i = tid; i < m; i += SOL_NT) {
            const double a = w.colc[i];
            if (fabs(a) <= ptol) continue;
            const int j = w.basic[i];
            const double room = a > 0 ? w.xB[i] - w.lo[j] : w.hi[j] - w.xB[i];
            tmax = fmin(tmax, (fmax(room, 0.0) + S_PTOL) / fabs(a));
        }
        tmax = block_min(sh, tmax);
        double av = -1.0; int ai = -1;
        for (int i = tid; i < m; i += SOL_NT) {
            const double a = w.colc[i];
            if (fabs(a) <= ptol) continue;
            const int j = w.basic[i];
            const double room = a > 0 ? w.xB[i] - w.lo[j] : w.hi[j] - w.xB[i];
            if (fmax(room, 0.0) / fabs(a) <= tmax && fabs(a) > av) { av = fabs(a); ai = i; }
        }
        const int r = block_argmax(sh, av, ai, &tmp);
        if (r < 0) {
            const double range = w.hi[jc] - w.lo[jc];
            if (!(range < S_INF)) return LP_UNBOUNDED;
            const double nw = w.at_upper[c] ? w.lo[jc] : w.hi[jc];
            const double dl = (nw - w.xN[c]) * dir;                      // colc holds D[:,c]*dir
            __syncthreads();
            for (int i = tid; i < m; i += SOL_NT) w.xB[i] -= w.colc[i] * dl;
            if (tid == 0) { w.xN[c] = nw; w.at_upper[c] = !w.at_upper[c]; sh.pivots++; }
            continue;
        }
        const int jr = w.basic[r];
        MLD_CHECK(w, r < m && c >= 0 && c < n && jr >= 0 && jr < n + w.mcap, 137, r, c);
        const double a_r = w.colc[r];
        s_pivot(w, sh, r, c, a_r > 0 ? w.lo[jr] : w.hi[jr]);
    }
}

// y = P x  (P: n x n row-major, shared per model and L2 resident); a wave per row
__device__ void s_matvecP(const Ws &w, const double *x, double *y)
{
    const int n = w.n, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    for (int i = wave; i < n; i += SOL_NW) {
        const double *pi = w.P + (size_t)i * n;
        double acc = 0.0;
        for (int j = lane; j < n; j += 64) acc += pi[j] * x[j];
        acc = wave_sum(acc);
        if (lane == 0) y[i] = acc;
    }
    __syncthreads();
}

__device__ double s_dot(Shared &sh, const double *a, const double *b, int n)
{
    double acc = 0.0;
    for (int j = threadIdx.x; j < n; j += SOL_NT) acc += a[j] * b[j];
    return block_sum(sh, acc);
}

// min 1/2 w'Hw + c'w over the unit simplex (p <= SD_PMAX): primal active set, executed by thread 0
// (its work arrays live in the slot -- `scr`, SD_MQ_DOUBLES doubles: as thread-private arrays they were 9.6 KB of scratch for EVERY lane of the kernel)
#define SD_MQ_DOUBLES ((SD_PMAX + 1) * (SD_PMAX + 2) + (SD_PMAX + 1) + SD_PMAX + SD_PMAX / 2 + SD_PMAX / 8)
__device__ void s_master_qp(int p, const double *H, const double *c, double *w, int enter, double *scr)
{
    double *K = scr, *sol = K + (SD_PMAX + 1) * (SD_PMAX + 2), *wn = sol + (SD_PMAX + 1);
    int *idx = (int *)(wn + SD_PMAX);
    unsigned char *F = (unsigned char *)(idx + SD_PMAX);
    for (int i = 0; i < p; ++i) F[i] = w[i] > 0 || i == enter;
    for (int iter = 0; iter < 200; ++iter) {
        int nf = 0;
        for (int i = 0; i < p; ++i) if (F[i]) idx[nf++] = i;
        const int N1 = nf + 1;
        double tr = 0; for (int a = 0; a < nf; ++a) tr += H[idx[a] * SD_PMAX + idx[a]];
        const double ridge = 1e-14 * fmax(tr, 1e-300);
        for (int a = 0; a < nf; ++a) {
            for (int b = 0; b < nf; ++b) K[a * (N1 + 1) + b] = H[idx[a] * SD_PMAX + idx[b]] + (a == b ? ridge : 0.0);
            K[a * (N1 + 1) + nf] = 1.0; K[a * (N1 + 1) + N1] = -c[idx[a]];
        }
        for (int b = 0; b < nf; ++b) K[nf * (N1 + 1) + b] = 1.0;
        K[nf * (N1 + 1) + nf] = 0.0; K[nf * (N1 + 1) + N1] = 1.0;
        for (int k = 0; k < N1; ++k) {
            int pv = k; double mx = fabs(K[k * (N1 + 1) + k]);
            for (int a = k + 1; a < N1; ++a) if (fabs(K[a * (N1 + 1) + k]) > mx) { mx = fabs(K[a * (N1 + 1) + k]); pv = a; }
            if (pv != k) for (int b = 0; b <= N1; ++b) { const double t2 = K[k * (N1 + 1) + b]; K[k * (N1 + 1) + b] = K[pv * (N1 + 1) + b]; K[pv * (N1 + 1) + b] = t2; }
            const double piv = K[k * (N1 + 1) + k];
            if (fabs(piv) < 1e-300) continue;
            for (int a = k + 1; a < N1; ++a) {
                const double f = K[a * (N1 + 1) + k] / piv;
                if (f != 0.0) for (int b = k; b <= N1; ++b) K[a * (N1 + 1) + b] -= f * K[k * (N1 + 1) + b];
            }
        }
        for (int k = N1 - 1; k >= 0; --k) {
            double sacc = K[k * (N1 + 1) + N1];
            for (int b = k + 1; b < N1; ++b) sacc -= K[k * (N1 + 1) + b] * sol[b];
            const double piv = K[k * (N1 + 1) + k];
            sol[k] = fabs(piv) < 1e-300 ? 0.0 : sacc / piv;
        }
        for (int i = 0; i < p; ++i) wn[i] = 0.0;
        for (int a = 0; a < nf; ++a) wn[idx[a]] = sol[a];
        int blocking = -1; double alpha = 1.0;
        for (int a = 0; a < nf; ++a) {
            const int i = idx[a];
            if (wn[i] < -1e-13 && w[i] - wn[i] > 0) { const double al = w[i] / (w[i] - wn[i]); if (al < alpha) { alpha = al; blocking = i; } }
        }
        if (blocking >= 0) {
            for (int i = 0; i < p; ++i) w[i] += alpha * (wn[i] - w[i]);
            w[blocking] = 0.0; F[blocking] = 0;
            continue;
        }
        for (int i = 0; i < p; ++i) w[i] = wn[i] > 0 ? wn[i] : 0.0;
        int add = -1; double worst = -1e-12;
        for (int i = 0; i < p; ++i) {
            if (F[i]) continue;
            double g = c[i]; for (int j = 0; j < p; ++j) g += H[i * SD_PMAX + j] * w[j];
            if (g + sol[nf] < worst) { worst = g + sol[nf]; add = i; }
        }
        if (add < 0) break;
        F[add] = 1;
    }
    double sw = 0; for (int i = 0; i < p; ++i) sw += w[i];
    if (sw > 0) for (int i = 0; i < p; ++i) w[i] /= sw;
}

// Convex-QP relaxation of the current node by simplicial decomposition (von Hohenbalken 1977).  On entry and on
// exit the dictionary is LP(q)-optimal for the node.  Returns 0 (bound in *lb_out, value in *fv_out, point in
// w.vcur), 1 if the bound already exceeds `cutoff`, -1 on an iteration limit.
__device__ int s_sd_relax(const Ws &w, Shared &sh, double cutoff, int max_pivots, double *lb_out, double *fv_out)
{
    const int n = w.n, tid = threadIdx.x;
    int p = 1, rc = 0;
    s_gather_x(w, sh, w.Y);
    s_matvecP(w, w.Y, w.PY);
    {
        const double hh = s_dot(sh, w.Y, w.PY, n), cc = s_dot(sh, w.qs, w.Y, n);
        if (tid == 0) { w.Hm[0] = hh; w.cm[0] = cc; w.wm[0] = 1.0; }
    }
    for (int j = tid; j < n; j += SOL_NT) { w.vcur[j] = w.Y[j]; w.Pv[j] = w.PY[j]; }
    __syncthreads();
    double LB = -S_INF, fv = 0.0;
    for (int it = 0; it < 80; ++it) {
        double a1 = 0.0, a2 = 0.0;
        for (int j = tid; j < n; j += SOL_NT) {
            const double g = w.Pv[j] + w.qs[j];
            w.gcost[j] = g;
            a1 += w.vcur[j] * (0.5 * w.Pv[j] + w.qs[j]);
            a2 += g * w.vcur[j];
        }
        fv = block_sum(sh, a1);
        const double gv = block_sum(sh, a2);
        s_reprice(w, sh, w.gcost);
        if (s_primal_simplex(w, sh, max_pivots) != LP_OPTIMAL) { rc = -2; break; }
        if (p >= SD_PMAX) {   // drop the lightest vertex (thread 0 edits the small arrays, all threads move the points)
            __syncthreads();
            int k = 0;
            for (int i = 1; i < p; ++i) if (w.wm[i] < w.wm[k]) k = i;
            for (int i = k; i + 1 < p; ++i)
                for (int j = tid; j < n; j += SOL_NT) { w.Y[(size_t)i * n + j] = w.Y[(size_t)(i + 1) * n + j]; w.PY[(size_t)i * n + j] = w.PY[(size_t)(i + 1) * n + j]; }
            __syncthreads();
            if (tid == 0) {
                for (int i = k; i + 1 < p; ++i) { w.wm[i] = w.wm[i + 1]; w.cm[i] = w.cm[i + 1]; }
                for (int a = 0; a < p; ++a) for (int b = k; b + 1 < p; ++b) w.Hm[a * SD_PMAX + b] = w.Hm[a * SD_PMAX + b + 1];
                for (int a = k; a + 1 < p; ++a) for (int b = 0; b < p; ++b) w.Hm[a * SD_PMAX + b] = w.Hm[(a + 1) * SD_PMAX + b];
            }
            p--;
            __syncthreads();
        }
        double *ynew = w.Y + (size_t)p * n;
        s_gather_x(w, sh, ynew);
        const double gy = s_dot(sh, w.gcost, ynew, n);
        const double lbt = fv + gy - gv;
        if (lbt > LB) LB = lbt;
        if (fv - LB <= 1e-10 * fmax(1.0, fabs(fv))) break;
        if (LB > cutoff) { rc = 1; break; }
        s_matvecP(w, ynew, w.PY + (size_t)p * n);
        for (int i = 0; i <= p; ++i) {
            const double hv = s_dot(sh, w.Y + (size_t)i * n, w.PY + (size_t)p * n, n);
            if (tid == 0) { w.Hm[i * SD_PMAX + p] = hv; w.Hm[p * SD_PMAX + i] = hv; }
        }
        {
            const double cc = s_dot(sh, w.qs, ynew, n);
            if (tid == 0) { w.cm[p] = cc; w.wm[p] = 0.0; }
        }
        p++;
        __syncthreads();
        if (tid == 0) {
            const long long tm0 = wall_clock64();
            s_master_qp(p, w.Hm, w.cm, w.wm, p - 1, w.mq);
            if (!w.dbg) sh.prof[7] += wall_clock64() - tm0;      // (QP batches: slot 7 = master problem)
            // drop zero-weight vertices from the small arrays; record the surviving source indices in sh.s_i
            int k2 = 0;
            for (int i = 0; i < p; ++i) {
                if (w.wm[i] <= 0.0) continue;
                if (k2 != i) {
                    w.wm[k2] = w.wm[i]; w.cm[k2] = w.cm[i];
                    for (int a = 0; a < p; ++a) w.Hm[a * SD_PMAX + k2] = w.Hm[a * SD_PMAX + i];
                    for (int b = 0; b < p; ++b) w.Hm[k2 * SD_PMAX + b] = w.Hm[i * SD_PMAX + b];
                }
                w.key[k2] = (double)i;          // source index of the k2-th survivor (key is free here)
                k2++;
            }
            sh.s_i[3] = k2;
        }
        __syncthreads();
        const int pn = sh.s_i[3];
        for (int k2 = 0; k2 < pn; ++k2) {
            const int src = (int)w.key[k2];
            if (src != k2)
                for (int j = tid; j < n; j += SOL_NT) { w.Y[(size_t)k2 * n + j] = w.Y[(size_t)src * n + j]; w.PY[(size_t)k2 * n + j] = w.PY[(size_t)src * n + j]; }
            __syncthreads();
        }
        p = pn;
        for (int j = tid; j < n; j += SOL_NT) {
            double a = 0.0, b = 0.0;
            for (int i = 0; i < p; ++i) { a += w.wm[i] * w.Y[(size_t)i * n + j]; b += w.wm[i] * w.PY[(size_t)i * n + j]; }
            w.vcur[j] = a; w.Pv[j] = b;
        }
        __syncthreads();
    }
    if (rc != -2) { s_reprice(w, sh, w.qs); if (s_primal_simplex(w, sh, max_pivots) != LP_OPTIMAL) rc = -2; }
    if (rc == -2) {
        // the primal simplex gave up (pivot limit, or cycling on a dictionary that has lost its accuracy): re-derive the dictionary from the original rows and
        // return to the LP(q) vertex of the node with the dual simplex; the caller goes on with the LP bound and the LP point of this node (-2), or ends (-1)
        __syncthreads();
        s_refactor(w, sh);
        __syncthreads();
        if (sh.pivots >= max_pivots || s_dual_simplex(w, sh, S_INF, max_pivots) != LP_OPTIMAL) rc = -1;
    }
    *lb_out = LB; *fv_out = fv;
    return rc;
}

// Closing sweep of the in-kernel hand-off under a quadratic cost: an open sibling whose LP(q) value did not pass the cutoff gets its QP relaxation.
// Closed only on a proven lower bound -- the simplicial-decomposition bound passed the cutoff (rc 1, or a finished bound above it); -1 (limit)
// leaves the node open, -2 (QP relaxation not finished) leaves the verdict to LP(q), which did not close it.  s_sd_relax returns with the
// dictionary's cost row at q and LP(q)-optimal for the node, as the node loop relies on.  Not inlined: the pivot loop's live ranges stay as they are.
__device__ __noinline__ bool s_sweep_close_qp(const Ws &w, Shared &sh, double sweep_cut, int max_pivots)
{
    double lbq, fvq;
    const int rc = s_sd_relax(w, sh, sweep_cut, max_pivots, &lbq, &fvq);
    return rc == 1 || (rc == 0 && lbq > sweep_cut);
}

// one round of Gomory mixed-integer cuts; returns the number added (same value on all threads)
__device__ __forceinline__ double wave_all_sum(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
__device__ __forceinline__ double wave_all_max(double v) { for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64)); return v; }
__device__ __forceinline__ double wave_all_min(double v) { for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64)); return v; }

// Gomory mixed-integer cuts of one round, SOL_NW at a time: the cuts of a round are independent of each other (they read the
// dictionary rows of fractional basics, never the rows appended in the same round), so every wave derives one cut on its own
// -- wave reductions, no block barrier -- in the per-wave lines the rounding cuts use for scoring (g in dictionary space, a in
// structural space), and the batch is committed in candidate order.  Candidates in the order the oracle takes them:
// |f0 - 1/2| ascending, row index on ties.  Same cuts, same order as the one-at-a-time version (s_gmi_round_serial).
#define GMI_KC 16
// the grouped slack substitution (every hot array in LDS): column chunks a lane accumulates in registers per pass (n <= 576: one pass) and slack rows
// whose loads are in flight together (GMI_GROUP x GMI_KC2 loads per lane)
#define GMI_KC2 9
#ifndef GMI_GROUP
#define GMI_GROUP 4
#endif
// a wave's own phases exchange data between lanes through its lines (LDS, or the slot when they do not fit): drain the wave's
// outstanding memory operations and keep the compiler from moving accesses across
#define WAVE_MEM_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_wave_barrier(); } while (0)
template <bool L>
__device__ __forceinline__ int s_gmi_round_t(const Ws &w, Shared &sh, int max_cuts)
{
    const int n = w.n, ld = w.ld, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    HOT_VIEW(L, w);
    (void)h_dw; (void)h_d; (void)h_skip;
    const typename CutT<L>::cu8p is_int = (typename CutT<L>::cu8p)w.is_int;
    const typename CutT<L>::u16p c_rowlist = (typename CutT<L>::u16p)w.rowlist, c_seclist = (typename CutT<L>::u16p)w.seclist;
    const typename HotT<L>::f64p c_colc = (typename HotT<L>::f64p)w.colc;
    const int m_start = sh.m;
    __syncthreads();
    // candidates (fractional integer basics), compacted in row order, then ranked by (key, row)
    int C = 0;
    for (int r0 = 0; r0 < m_start; r0 += SOL_NT) {
        const int r = r0 + tid;
        bool cand = false; double key = S_INF;
        if (r < m_start) {
            const int j = h_basic[r];
            if (j < n && is_int[j]) {
                const double f0 = h_xB[r] - floor(h_xB[r]);
                if (f0 > 1e-3 && f0 < 1 - 1e-3) { cand = true; key = fabs(f0 - 0.5); }
            }
            w.key[r] = key;
        }
        C = block_compact(sh, cand, (unsigned short)r, w.rowlist, C);
    }
    s_gather_x(w, sh, w.tmpx);
    MLD_CHECK(w, C <= m_start && m_start <= w.mcap && C <= (int)(w.rowlist - w.seclist), 116, C, m_start);
    for (int t = tid; t < C; t += SOL_NT) c_colc[t] = w.key[c_rowlist[t]];
    __syncthreads();
    for (int t = tid; t < C; t += SOL_NT) {
        const int r = c_rowlist[t];
        const double k = c_colc[t];
        int rank = 0;
        for (int u = 0; u < C; ++u) { const int ru = c_rowlist[u]; const double ku = c_colc[u]; rank += (ku < k) || (ku == k && ru < r); }
        c_seclist[rank] = (unsigned short)r;
    }
    __syncthreads();
    const typename HotT<L>::f64p gw = (typename HotT<L>::f64p)w.mir_cache + (size_t)wave * 2 * n, axw = gw + n;
    int added = 0;
    for (int pos = 0; pos < C; pos += SOL_NW) {
        if (m_start + added >= sh.cut_cap || added >= max_cuts) break;
        const int t = pos + wave;
        bool ok = t < C;
        double bx = 0.0, nrm = 0.0;
        if (ok) {
            const int r = c_seclist[t];
            const double f0 = h_xB[r] - floor(h_xB[r]);
            const glb_f64 *row = (const glb_f64 *)(w.D + (size_t)r * ld);
            double gmin = S_INF, gmax = 0.0;
            for (int c0 = 0; c0 < n; c0 += 512) {      // eight independent loads of the dictionary row in flight
            double rv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) { const int c = c0 + q * 64 + lane; rv[q] = c < n ? row[c] : 0.0; }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c = c0 + q * 64 + lane;
                if (c >= n) continue;
                const int j = h_nonbasic[c];
                double a = (h_lo[j] == h_hi[j]) ? 0.0 : (h_up[c] ? -rv[q] : rv[q]);
                // Coefficients below 1e-9 are dropped (round-off of the dictionary).  Dropping strengthens the cut by |a| t_j: harmless for a column
                // whose displacement t_j is O(1), NOT for a free variable resting on the artificial box (t_j up to 2e7): such a cut is not derived.
                bool unsafe = false;
                if (fabs(a) < S_COEF_ZERO) { unsafe = a != 0.0 && j < n && fabs(h_up[c] ? h_hi[j] : h_lo[j]) >= 0.5 * S_BIG; a = 0.0; }
                double gc;
                if (j < n && is_int[j]) {
                    double fj = a - floor(a);
                    if (fj < S_COEF_ZERO || fj > 1 - S_COEF_ZERO) fj = 0.0;
                    gc = fj <= f0 ? fj / f0 : (1 - fj) / (1 - f0);
                } else gc = a > 0 ? a / f0 : -a / (1 - f0);
                gw[c] = gc;
                axw[c] = 0.0;
                if (gc > 0) { gmin = fmin(gmin, gc); gmax = fmax(gmax, gc); }
                if (unsafe) { gmin = 0.0; gmax = fmax(gmax, 1.0); }      // rejected by the dynamic-range test below
            }
            }
            gmin = wave_all_min(gmin); gmax = wave_all_max(gmax);
            ok = (gmax > 0.0) && !(gmax / gmin > 1e6);
            WAVE_MEM_SYNC();
            if (ok) {
                // cut  sum_c g_c t_c >= 1  over structural variables:  ax.x <= bx
                double bx_part = 0.0;
                for (int c = lane; c < n; c += 64) {
                    const double gc = gw[c];
                    if (gc <= 0) continue;
                    const int j = h_nonbasic[c];
                    const double sg = h_up[c] ? -1.0 : 1.0;
                    if (j < n) { const double bnd = h_up[c] ? h_hi[j] : h_lo[j]; axw[j] = -gc * sg; bx_part -= gc * sg * bnd; }
                    else bx_part += gc * (j - n < w.m0 ? ((typename CutT<L>::cf64p)w.hs)[j - n] : ((typename CutT<L>::cf64p)w.hc)[j - n - w.m0]);      // (orig_rhs)
                }
                WAVE_MEM_SYNC();
                if constexpr (L) {
                // slack columns: ax += g_c * (original row of that slack), ascending c -- the same sequence of acc += g_c * value per structural column as the
                // round-4 loop below, but GMI_GROUP slack rows at a time: the set columns are taken in ascending order across the 64-column chunks, the loads
                // of all rows of a group are issued before the first multiply-add (one memory latency per group instead of one per slack column), and the rows
                // are read through global pointers (w.Gs / w.Gc: address space known), g_c and the column's variable through the LDS views
                const glb_f64 *Gs = (const glb_f64 *)w.Gs, *Gc = (const glb_f64 *)w.Gc;
                const int m0 = w.m0;
                for (int k0 = 0; k0 < n; k0 += 64 * GMI_KC2) {
                    double acc[GMI_KC2];
#pragma unroll
                    for (int q = 0; q < GMI_KC2; ++q) { const int k = k0 + q * 64 + lane; acc[q] = k < n ? axw[k] : 0.0; }
                    int c0 = 0;
                    unsigned long long mask = __ballot(lane < n && h_nonbasic[lane < n ? lane : 0] >= n && gw[lane < n ? lane : 0] > 0);
                    for (;;) {
                        int ri[GMI_GROUP]; double gs[GMI_GROUP];
#pragma unroll
                        for (int u = 0; u < GMI_GROUP; ++u) {
                            while (!mask && c0 + 64 < n) {
                                c0 += 64;
                                const int c = c0 + lane, cc = c < n ? c : 0;
                                mask = __ballot(c < n && h_nonbasic[cc] >= n && gw[cc] > 0);
                            }
                            ri[u] = -1; gs[u] = 0.0;
                            if (mask) {
                                const int cs = c0 + __ffsll((long long)mask) - 1;       // wave-uniform
                                mask &= mask - 1ull;
                                gs[u] = gw[cs];
                                ri[u] = __builtin_amdgcn_readfirstlane(h_nonbasic[cs]) - n;
                                MLD_CHECK(w, ri[u] >= 0 && ri[u] < m_start, 119, ri[u] + n, m_start);
                            }
                        }
                        if (ri[0] < 0) break;
                        double v[GMI_GROUP][GMI_KC2];
#pragma unroll
                        for (int u = 0; u < GMI_GROUP; ++u) {
                            const int i = ri[u] < 0 ? 0 : ri[u];
                            const glb_f64 *orow = i < m0 ? Gs + (size_t)i * n : Gc + (size_t)(i - m0) * n;
#pragma unroll
                            for (int q = 0; q < GMI_KC2; ++q) { const int k = k0 + q * 64 + lane; v[u][q] = (ri[u] >= 0 && k < n) ? orow[k] : 0.0; }
                        }
#pragma unroll
                        for (int u = 0; u < GMI_GROUP; ++u) {
                            if (ri[u] < 0) continue;
#pragma unroll
                            for (int q = 0; q < GMI_KC2; ++q) if (k0 + q * 64 < n) acc[q] += gs[u] * v[u][q];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < GMI_KC2; ++q) { const int k = k0 + q * 64 + lane; if (k < n) axw[k] = acc[q]; }
                }
                } else {
                // slack columns: ax += g_c * (original row of that slack), ascending c; a chunk of 64 * GMI_KC structural columns
                // is accumulated in registers, 16 independent loads per slack row
                for (int k0 = 0; k0 < n; k0 += 64 * GMI_KC) {
                    double acc[GMI_KC];
#pragma unroll
                    for (int q = 0; q < GMI_KC; ++q) { const int k = k0 + q * 64 + lane; acc[q] = k < n ? axw[k] : 0.0; }
                    for (int c0 = 0; c0 < n; c0 += 64) {
                        const int c = c0 + lane;
                        int jn = 0; double gc = 0.0;
                        if (c < n) { jn = h_nonbasic[c]; gc = gw[c]; }
                        unsigned long long mask = __ballot(c < n && jn >= n && gc > 0);
                        while (mask) {
                            const int src = __ffsll((long long)mask) - 1;
                            mask &= mask - 1ull;
                            const double gs = __shfl(gc, src, 64);
                            MLD_CHECK(w, __shfl(jn, src, 64) - n >= 0 && __shfl(jn, src, 64) - n < m_start, 119, __shfl(jn, src, 64), m_start);
                            const double *orow = orig_row(w, __shfl(jn, src, 64) - n);
#pragma unroll
                            for (int q = 0; q < GMI_KC; ++q) { const int k = k0 + q * 64 + lane; if (k0 + q * 64 < n) acc[q] += gs * (k < n ? orow[k] : 0.0); }
                        }
                    }
#pragma unroll
                    for (int q = 0; q < GMI_KC; ++q) { const int k = k0 + q * 64 + lane; if (k < n) axw[k] = acc[q]; }
                }
                }
                WAVE_MEM_SYNC();
                bx = wave_all_sum(bx_part) - 1.0;
                double nm = 0.0;
                for (int k = lane; k < n; k += 64) nm = fmax(nm, fabs(axw[k]));
                nrm = wave_all_max(nm);
                ok = nrm > 0.0;
                nrm = fmax(nrm, gmax);       // keep the dictionary row (coefficients g) O(1) as well as the structural row
#ifdef MLD_CUT_PROF
                int nsl = 0;
                for (int c0 = 0; c0 < n; c0 += 64) { const int c = c0 + lane, cc = c < n ? c : 0; nsl += __popcll(__ballot(c < n && h_nonbasic[cc] >= n && gw[cc] > 0)); }
                CUT_COUNT(sh, 5, nsl);
                CUT_COUNT(sh, 4, 1);
#endif
            }
        }
        if (lane == 0) sh.s_i[wave] = ok ? 1 : 0;
        __syncthreads();
        int before = 0, total = 0;
        for (int u = 0; u < SOL_NW; ++u) { const int f = sh.s_i[u]; if (u < wave) before += f; total += f; }
        const int room = min(sh.cut_cap - (m_start + added), max_cuts - added);
        if (ok && before < room) {
            const int kc = m_start + added + before;            // new row index
            MLD_CHECK(w, kc >= w.m0 && kc < w.mcap, 117, kc, added);
            const typename CutT<L>::gf64p gk = (typename CutT<L>::gf64p)(w.Gc + (size_t)(kc - w.m0) * n), dk = (typename CutT<L>::gf64p)(w.D + (size_t)kc * ld);
            const typename CutT<L>::cf64p tmpx = (typename CutT<L>::cf64p)w.tmpx;
            double sp = 0.0, dp = 0.0;
            for (int k = lane; k < n; k += 64) {
                const double a = axw[k] / nrm;
                gk[k] = a;
                sp += a * tmpx[k];
                const double sg = h_up[k] ? -1.0 : 1.0;
                const double dv = -(gw[k] / nrm) * sg;
                dk[k] = dv;
                dp += dv * h_xN[k];
            }
            const double s_now = bx / nrm - wave_all_sum(sp);
            const double dsum = wave_all_sum(dp);
            if (lane == 0) {
                w.hc[kc - w.m0] = bx / nrm;
                dk[n] = s_now + dsum;
                h_basic[kc] = n + kc; w.where[n + kc] = -1 - kc;
                h_xB[kc] = s_now;
                h_lo[n + kc] = 0.0; h_hi[n + kc] = S_INF;
            }
        }
        added += total < room ? total : room;
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) sh.m = m_start + added;
    __syncthreads();
    return added;
}

// the typed, grouped instantiation when every hot array and the per-wave lines are in LDS (the bench shapes); MLD_DBG_CUTS_R4 keeps round 4's
__device__ int s_gmi_round(const Ws &w, Shared &sh, int max_cuts)
{
    return (w.all_lds && w.mir_in_lds && !(w.dbg & MLD_DBG_CUTS_R4)) ? s_gmi_round_t<true>(w, sh, max_cuts) : s_gmi_round_t<false>(w, sh, max_cuts);
}

__device__ int s_gmi_round_serial(const Ws &w, Shared &sh, int max_cuts)
{
    const int n = w.n, ld = w.ld, tid = threadIdx.x;
    const int m_start = sh.m;
    __syncthreads();
    // keys: |f0 - 0.5| for fractional integer basics, +inf otherwise
    for (int r = tid; r < m_start; r += SOL_NT) {
        const int j = w.basic[r];
        double key = S_INF;
        if (j < n && w.is_int[j]) {
            const double f0 = w.xB[r] - floor(w.xB[r]);
            if (f0 > 1e-3 && f0 < 1 - 1e-3) key = fabs(f0 - 0.5);
        }
        w.key[r] = key;
    }
    s_gather_x(w, sh, w.tmpx);
    int added = 0;
    for (;;) {
        __syncthreads();
        if (m_start + added >= sh.cut_cap || added >= max_cuts) break;
        // next candidate: smallest key, smallest row index on ties
        double myv = -S_INF; int myi = -1;
        for (int r = tid; r < m_start; r += SOL_NT) { const double k = -w.key[r]; if (k > myv) { myv = k; myi = r; } }
        double bv;
        const int r = block_argmax(sh, myv, myi, &bv);
        if (r < 0 || bv == -S_INF) break;
        __syncthreads();
        if (tid == 0) w.key[r] = S_INF;
        const double f0 = w.xB[r] - floor(w.xB[r]);
        const double *row = w.D + (size_t)r * ld;
        double gmin = S_INF, gmax = 0.0;
        for (int c = tid; c < n; c += SOL_NT) {
            const int j = w.nonbasic[c];
            double a = (w.lo[j] == w.hi[j]) ? 0.0 : (w.at_upper[c] ? -row[c] : row[c]);
            bool unsafe = false;      // (see the wave-parallel round: a dropped coefficient on a column resting on the artificial box)
            if (fabs(a) < S_COEF_ZERO) { unsafe = a != 0.0 && j < n && fabs(w.at_upper[c] ? w.hi[j] : w.lo[j]) >= 0.5 * S_BIG; a = 0.0; }
            double gc;
            if (j < n && w.is_int[j]) {
                double fj = a - floor(a);
                if (fj < S_COEF_ZERO || fj > 1 - S_COEF_ZERO) fj = 0.0;
                gc = fj <= f0 ? fj / f0 : (1 - fj) / (1 - f0);
            } else gc = a > 0 ? a / f0 : -a / (1 - f0);
            w.g[c] = gc;
            if (gc > 0) { gmin = fmin(gmin, gc); gmax = fmax(gmax, gc); }
            if (unsafe) { gmin = 0.0; gmax = fmax(gmax, 1.0); }
        }
        gmin = block_min(sh, gmin);
        gmax = block_max(sh, gmax);
        if (!(gmax > 0.0) || gmax / gmin > 1e6) continue;
        // cut  sum_c g_c t_c >= 1  over structural variables:  ax.x <= bx
        for (int j = tid; j < n; j += SOL_NT) w.ax[j] = 0.0;
        __syncthreads();
        double bx_part = 0.0;
        for (int c = tid; c < n; c += SOL_NT) {
            const double gc = w.g[c];
            if (gc <= 0) continue;
            const int j = w.nonbasic[c];
            const double sg = w.at_upper[c] ? -1.0 : 1.0;
            if (j < n) { const double bnd = w.at_upper[c] ? w.hi[j] : w.lo[j]; w.ax[j] = -gc * sg; bx_part -= gc * sg * bnd; }
            else bx_part += gc * orig_rhs(w, j - n);
        }
        __syncthreads();
        // slack columns: ax += g_c * (original row of that slack).  The (row, g) pairs are compacted into LDS first,
        // then threads own structural indices k and keep 4 row loads in flight.
        int nsl = 0;
        for (int c0 = 0; c0 < n; c0 += SOL_NT) {
            const int c = c0 + tid;
            const bool f = c < n && w.nonbasic[c] >= n && w.g[c] > 0;
            nsl = block_compact(sh, f, (unsigned short)c, w.rowlist, nsl);      // column indices, ascending
        }
        __syncthreads();
        for (int t = tid; t < nsl; t += SOL_NT) { const int c = w.rowlist[t]; w.colc[t] = w.g[c]; w.seclist[t] = (unsigned short)(w.nonbasic[c] - n); }
        __syncthreads();
        {
            for (int k = tid; k < n; k += SOL_NT) {
                double acc = w.ax[k];
                int t = 0;
                for (; t + 4 <= nsl; t += 4) {
                    const double v0 = orig_row(w, w.seclist[t])[k], v1 = orig_row(w, w.seclist[t + 1])[k],
                                 v2 = orig_row(w, w.seclist[t + 2])[k], v3 = orig_row(w, w.seclist[t + 3])[k];
                    acc += w.colc[t] * v0; acc += w.colc[t + 1] * v1; acc += w.colc[t + 2] * v2; acc += w.colc[t + 3] * v3;
                }
                for (; t < nsl; ++t) acc += w.colc[t] * orig_row(w, w.seclist[t])[k];
                w.ax[k] = acc;
            }
        }
        __syncthreads();
        const double bx = block_sum(sh, bx_part) - 1.0;
        double nm = 0.0;
        for (int k = tid; k < n; k += SOL_NT) nm = fmax(nm, fabs(w.ax[k]));
        double nrm = block_max(sh, nm);
        if (!(nrm > 0.0)) continue;
        nrm = fmax(nrm, gmax);       // keep the dictionary row (coefficients g) O(1) as well as the structural row
        const int kc = m_start + added;            // new row index
        double *gk = w.Gc + (size_t)(kc - w.m0) * n, *dk = w.D + (size_t)kc * ld;
        double sp = 0.0, dp = 0.0;
        for (int k = tid; k < n; k += SOL_NT) {
            const double a = w.ax[k] / nrm;
            gk[k] = a;
            sp += a * w.tmpx[k];
            const double sg = w.at_upper[k] ? -1.0 : 1.0;
            const double dv = -(w.g[k] / nrm) * sg;
            dk[k] = dv;
            dp += dv * w.xN[k];
        }
        const double s_now = bx / nrm - block_sum(sh, sp);
        const double dsum = block_sum(sh, dp);
        if (tid == 0) {
            w.hc[kc - w.m0] = bx / nrm;
            dk[n] = s_now + dsum;
            w.basic[kc] = n + kc; w.where[n + kc] = -1 - kc;
            w.xB[kc] = s_now;
            w.lo[n + kc] = 0.0; w.hi[n + kc] = S_INF;
        }
        added++;
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) sh.m = m_start + added;
    __syncthreads();
    return added;
}

// ---- complemented mixed-integer rounding cuts on the ORIGINAL rows (oracle/mld_oracle.c mir_round) -------------------
// A wave owns a row: pass 1 bound-substitutes the continuous entries and complements binaries above 1/2 (right-hand side,
// continuous slack value and norm), caching the free binaries' coefficients in a per-wave LDS/HBM line; every candidate
// divisor delta = |g_j| / {1,2,4,8} of a fractional binary of the row is then scored on the cached line only.
// scores the four divisors d0 / {1,2,4,8} in one sweep over the wave's compact list of the row's free binaries
// (ga = complemented coefficient, gx = complemented value); updates (best, bdelta) in the oracle's order q = 0..3
template <typename GB>
__device__ __forceinline__ void s_mir_score4(GB ga, GB gx, int cnt, int lane, double rhs, double sval, double S2, double d0,
                                             double &best, double &bdelta)
{
    double f[4], fb[4], inv1f[4], lhs[4], nrm2[4]; bool use[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double delta = d0 / (double)(1 << q);
        const double b = rhs / delta;
        fb[q] = floor(b); f[q] = b - fb[q];
        use[q] = delta >= 1e-9 && f[q] >= S_MIR_FMIN && f[q] <= 1.0 - S_MIR_FMIN;
        inv1f[q] = 1.0 / (1.0 - f[q]);
        lhs[q] = 0.0; nrm2[q] = 0.0;
    }
    if (!(use[0] || use[1] || use[2] || use[3])) return;
    for (int t = lane; t < cnt; t += 64) {
        const double a0 = ga[t], x = gx[t];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double a = a0 / (d0 / (double)(1 << q)), fl = floor(a + 1e-12), fj = a - fl;
            const double cf = fl + (fj > f[q] ? (fj - f[q]) * inv1f[q] : 0.0);
            lhs[q] += cf * x;
            nrm2[q] += cf * cf;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double l = wave_sum(lhs[q]), m2 = wave_sum(nrm2[q]);
        l = __shfl(l, 0, 64); m2 = __shfl(m2, 0, 64);
        if (!use[q]) continue;
        const double delta = d0 / (double)(1 << q), kc = inv1f[q] / delta;
        const double viol = l - sval * kc - fb[q];
        m2 += kc * kc * S2;
        if (viol <= 1e-6 || !(m2 > 0.0)) continue;
        const double eff = viol / sqrt(m2);
        if (eff > best) { best = eff; bdelta = delta; }
    }
}

// The same scores with the wave split into 64 / W sub-groups of W lanes (W = 32 for a list of at most 32 entries, 16 for at most 16): every sub-group
// scores another divisor of the row, 64 / W fractional binaries of `mask` (ascending) at a time.  Bit for bit the results of s_mir_score4 one divisor
// after the other:
//  * per entry and q the same operations (the four divisions a0 / (d0 / 2^q) are kept as they are);
//  * wave_sum is v += shfl_down(v, o) for o = 32 .. 1, and there every lane from cnt on holds +0.0 (its sum never started) while no partial sum is -0.0
//    (each starts from +0.0), so the steps o >= W add +0.0 to what lane 0 ends with and the steps o < W read lanes below W only: the same tree run
//    from o = W / 2 gives a sub-group's first lane exactly that value;
//  * (best, bdelta) takes "the first strictly greater" in the order (divisor ascending, q ascending): a sub-group keeps the first strictly greater of
//    its q = 0 .. 3 (every efficacy that gets there is > 0), the sub-groups are then taken in ascending divisor order with the same strict test -- the
//    first occurrence of the maximum either way.
template <int W, typename GB>
__device__ __forceinline__ void s_mir_score_sub(GB ga, GB gx, int cnt, int lane, double rhs, double sval, double S2, unsigned long long mask,
                                                double &best, double &bdelta)
{
    const int sub = lane / W, sl = lane % W;
    double a0 = 0.0, x = 0.0;
    if (sl < cnt) { a0 = ga[sl]; x = gx[sl]; }
    while (mask) {
        int src = -1;
#pragma unroll
        for (int g = 0; g < 64 / W; ++g) if (mask) { const int s1 = __ffsll((long long)mask) - 1; mask &= mask - 1ull; if (sub == g) src = s1; }
        const bool act = src >= 0;
        const double d0 = fabs(__shfl(a0, act ? src : 0, 64));
        double f[4], fb[4], inv1f[4], lhs[4], nrm2[4]; bool use[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double delta = d0 / (double)(1 << q);
            const double b = rhs / delta;
            fb[q] = floor(b); f[q] = b - fb[q];
            use[q] = act && delta >= 1e-9 && f[q] >= S_MIR_FMIN && f[q] <= 1.0 - S_MIR_FMIN;
            inv1f[q] = 1.0 / (1.0 - f[q]);
            lhs[q] = 0.0; nrm2[q] = 0.0;
        }
        if (sl < cnt && (use[0] || use[1] || use[2] || use[3])) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double a = a0 / (d0 / (double)(1 << q)), fl = floor(a + 1e-12), fj = a - fl;
                const double cf = fl + (fj > f[q] ? (fj - f[q]) * inv1f[q] : 0.0);
                lhs[q] += cf * x;
                nrm2[q] += cf * cf;
            }
        }
        double le = 0.0, ld = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double l = lhs[q], m2 = nrm2[q];
#pragma unroll
            for (int o = W / 2; o > 0; o >>= 1) { l += __shfl_down(l, o, 64); m2 += __shfl_down(m2, o, 64); }
            l = __shfl(l, sub * W, 64); m2 = __shfl(m2, sub * W, 64);
            if (!use[q]) continue;
            const double delta = d0 / (double)(1 << q), kc = inv1f[q] / delta;
            const double viol = l - sval * kc - fb[q];
            m2 += kc * kc * S2;
            if (viol <= 1e-6 || !(m2 > 0.0)) continue;
            const double eff = viol / sqrt(m2);
            if (eff > le) { le = eff; ld = delta; }
        }
#pragma unroll
        for (int g = 0; g < 64 / W; ++g) {
            const double eg = __shfl(le, g * W, 64), dg = __shfl(ld, g * W, 64);
            if (eg > best) { best = eg; bdelta = dg; }
        }
    }
}

// every candidate divisor of a row whose compact list is built (ascending j, as the oracle enumerates them): best efficacy and its divisor
template <typename GB>
__device__ __forceinline__ void s_mir_score_row(GB ga, GB gx, int cnt, int lane, double rhs, double sval, double S2, int usable, bool split, Shared &sh,
                                                double &best, double &bdelta)
{
    best = 0.0; bdelta = 0.0;
#ifdef MLD_CUT_PROF
    if (__ballot(!usable) == 0ull) {
        int nd = 0;
        for (int t0 = 0; t0 < cnt; t0 += 64) { const int t = t0 + lane; bool fr = false; if (t < cnt) { const double x = gx[t]; fr = x > 1e-6 && x < 1 - 1e-6; } nd += __popcll(__ballot(fr)); }
        CUT_COUNT(sh, 8, 1); CUT_COUNT(sh, 9, cnt); CUT_COUNT(sh, 10, nd);
    }
#endif
    if (__ballot(!usable) == 0ull && split && cnt <= 32) {
        // (a list of at most 32 entries -- every row of the bench shape -- leaves half or three quarters of the wave idle: two or four divisors at once)
        bool fr = false;
        if (lane < cnt) { const double x = gx[lane]; fr = x > 1e-6 && x < 1 - 1e-6; }
        const unsigned long long mask = __ballot(fr);
        if (cnt <= 16) s_mir_score_sub<16>(ga, gx, cnt, lane, rhs, sval, S2, mask, best, bdelta);
        else s_mir_score_sub<32>(ga, gx, cnt, lane, rhs, sval, S2, mask, best, bdelta);
    } else
    if (__ballot(!usable) == 0ull) {
        for (int t0 = 0; t0 < cnt; t0 += 64) {           // candidate divisors in ascending j, as the oracle enumerates them
            const int t = t0 + lane;
            double a0 = 0.0; bool fr = false;
            if (t < cnt) { a0 = ga[t]; const double x = gx[t]; fr = x > 1e-6 && x < 1 - 1e-6; }
            unsigned long long mask = __ballot(fr);
            while (mask) {
                const int src = __ffsll((long long)mask) - 1;
                mask &= mask - 1ull;
                const double d0 = fabs(__shfl(a0, src, 64));
                s_mir_score4(ga, gx, cnt, lane, rhs, sval, S2, d0, best, bdelta);
            }
        }
    }
}

template <typename GB>
__device__ __forceinline__ void s_mir_phase_a(GB ga, GB gx, int cap, const Ws &w, const lds_f64 *xs, int ncand, int wave, int lane, bool split, Shared &sh)
{
    const int n = w.n;
    const lds_u16 *rows = (const lds_u16 *)w.rowlist;
    for (int qi = wave; qi < ncand; qi += SOL_NW) {
        const int i = rows[qi];
#ifdef MLD_CUT_PROF
        const long long tp1 = wall_clock64();
#endif
        MLD_CHECK(w, i >= 0 && i < w.m0 && cap > 0, 125, i, cap);
        const double *g = w.Gs + (size_t)i * n;
        // pass 1: bound substitution of the continuous entries, complementing of binaries above 1/2; the free binaries are
        // compacted (ascending j) into the wave's list
        double rhs = 0.0, sval = 0.0, S2 = 0.0; int usable = 1, cnt = 0;
        // the condensed rows are causal (block lower triangular H_v): row i of step k = i / nc has no entry beyond step k
        const int jmax = w.nc_step > 0 ? min(n, (i / w.nc_step + 1) * w.nv_step) : n;
        bool over = false;       // wave-uniform
        if (w.csr_ptr) {
            // (round 4) the row's entries from the sparse copy, a lane per entry, 64 at a time: ascending column order like the dense walk below, so the compacted
            // list -- and every cut -- is the same; a cfg4 row has 11 entries on average where the dense walk loaded half a row of 575
            (void)jmax;
            const int e0 = w.csr_ptr[i], e1 = w.csr_ptr[i + 1];
            for (int eb = e0; eb < e1 && !over; eb += 64) {
                const int e = eb + lane;
                bool keep = false; double ac = 0.0, xc = 0.0;
                if (e < e1) {
                    const int j = w.csr_col[e];
                    const double gj = w.csr_val[e];
                    const double x = xs[j];
                    if (w.is_int[j]) {
                        const double lo = w.lo[j], hi = w.hi[j];
                        if (lo == hi) rhs -= gj * lo;
                        else { const bool comp = x > 0.5; if (comp) rhs -= gj; keep = true; ac = comp ? -gj : gj; xc = comp ? 1.0 - x : x; }
                    } else {
                        const double lo = w.clo[j], hi = w.chi[j];
                        const bool lof = lo > -0.5 * S_BIG, hif = hi < 0.5 * S_BIG;
                        if (gj > 0) { if (lof) rhs -= gj * lo; else if (hif) { rhs -= gj * hi; sval += gj * (hi - x); S2 += gj * gj; } else usable = 0; }
                        else { if (lof) { rhs -= gj * lo; sval += -gj * (x - lo); S2 += gj * gj; } else if (hif) rhs -= gj * hi; else usable = 0; }
                    }
                }
                const unsigned long long bal = __ballot(keep);
                if (cnt + __popcll(bal) > cap) { usable = 0; over = true; break; }
                if (keep) { const int pos = cnt + __popcll(bal & ((1ull << lane) - 1ull)); ga[pos] = ac; gx[pos] = xc; }
                cnt += __popcll(bal);
            }
        } else
        for (int j0 = 0; j0 < jmax && !over; j0 += 256) {
            double gq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int j = j0 + q * 64 + lane; gq[q] = j < jmax ? g[j] : 0.0; }   // 4 independent loads in flight
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = j0 + q * 64 + lane;
                if (j0 + q * 64 >= jmax) break;
                bool keep = false; double ac = 0.0, xc = 0.0;
                const double gj = gq[q];
                if (gj != 0.0) {
                    const double x = xs[j];
                    if (w.is_int[j]) {
                        const double lo = w.lo[j], hi = w.hi[j];
                        if (lo == hi) rhs -= gj * lo;
                        else { const bool comp = x > 0.5; if (comp) rhs -= gj; keep = true; ac = comp ? -gj : gj; xc = comp ? 1.0 - x : x; }
                    } else {
                        const double lo = w.clo[j], hi = w.chi[j];      // (implied bounds of the presolve where it ran)
                        const bool lof = lo > -0.5 * S_BIG, hif = hi < 0.5 * S_BIG;
                        if (gj > 0) { if (lof) rhs -= gj * lo; else if (hif) { rhs -= gj * hi; sval += gj * (hi - x); S2 += gj * gj; } else usable = 0; }
                        else { if (lof) { rhs -= gj * lo; sval += -gj * (x - lo); S2 += gj * gj; } else if (hif) rhs -= gj * hi; else usable = 0; }
                    }
                }
                const unsigned long long bal = __ballot(keep);
                if (cnt + __popcll(bal) > cap) { usable = 0; over = true; break; }      // (cannot happen: cap counts the integer entries of the widest original row)
                if (keep) { const int pos = cnt + __popcll(bal & ((1ull << lane) - 1ull)); ga[pos] = ac; gx[pos] = xc; }
                cnt += __popcll(bal);
            }
        }
        rhs = wave_sum(rhs); sval = wave_sum(sval); S2 = wave_sum(S2);
        rhs = __shfl(rhs, 0, 64) + w.hs[i]; sval = __shfl(sval, 0, 64); S2 = __shfl(S2, 0, 64);
        double best, bdelta;
#ifdef MLD_CUT_PROF
        const long long tp2 = wall_clock64();
        if (wave == 0 && lane == 0) sh.cprof[13] += tp2 - tp1;
#endif
        s_mir_score_row(ga, gx, cnt, lane, rhs, sval, S2, usable, split, sh, best, bdelta);
        if (lane == 0) { w.mir_eff[i] = best > 1e-4 ? best : -S_INF; w.mir_delta[i] = bdelta; }
#ifdef MLD_CUT_PROF
        if (wave == 0 && lane == 0) sh.cprof[14] += wall_clock64() - tp2;
#endif
    }
}

// Phase A over the sparse copy with the row a wave takes next in flight (the path of every handle that has the copy; MLD_DBG_WALKS_SERIAL keeps the loop
// above).  A scored row was a chain of dependent round trips -- rowlist -> csr_ptr -> (column, value) -> is_int -> bounds, then hs after the wave sums.  Here
// the csr_ptr pair and hs of row qi + SOL_NW are loaded while row qi is processed, its first 64 entries are issued before row qi's divisor loop starts, and
// is_int / clo / chi are loaded together behind the column index (the LP bounds of a binary come from LDS when L).  Typed views: global_* for the instance
// data, ds_* for the workgroup's lists.  A wave without a next row re-reads its own row's pair (nothing past ncand or csr_ptr[m0] is read).  Per row the
// same operations on the same operands in the same order as above.
template <typename GB, bool L>
__device__ __forceinline__ void s_mir_phase_a_pipe(GB ga, GB gx, int cap, const Ws &w, const lds_f64 *xs, int ncand, int wave, int lane, bool split, Shared &sh)
{
    const lds_u16 *rows = (const lds_u16 *)w.rowlist;
    glb_ci32 *ptr = (glb_ci32 *)w.csr_ptr; glb_cu16 *col = (glb_cu16 *)w.csr_col; glb_cf64 *val = (glb_cf64 *)w.csr_val;
    glb_cf64 *ghs = (glb_cf64 *)w.hs, *gclo = (glb_cf64 *)w.clo, *gchi = (glb_cf64 *)w.chi;
    const typename CutT<true>::cu8p isint = (typename CutT<true>::cu8p)w.is_int;
    const typename HotT<L>::f64p h_lo = (typename HotT<L>::f64p)w.lo, h_hi = (typename HotT<L>::f64p)w.hi;
    if (wave >= ncand) return;
    int i = rows[wave];
    int e0 = ptr[i], e1 = ptr[i + 1];
    double hsv = ghs[i];
    int jf = 0; double gf = 0.0;
    if (e0 + lane < e1) { jf = col[e0 + lane]; gf = val[e0 + lane]; }
    for (int qi = wave; qi < ncand; qi += SOL_NW) {
#ifdef MLD_CUT_PROF
        const long long tp1 = wall_clock64();
#endif
        MLD_CHECK(w, i >= 0 && i < w.m0 && cap > 0, 125, i, cap);
        const bool has = qi + SOL_NW < ncand;
        const int in = has ? (int)rows[qi + SOL_NW] : i;
        const int e0n = ptr[in], e1n = ptr[in + 1];
        const double hsn = ghs[in];
        double rhs = 0.0, sval = 0.0, S2 = 0.0; int usable = 1, cnt = 0;
        bool over = false;       // wave-uniform
        for (int eb = e0; eb < e1 && !over; eb += 64) {
            const int e = eb + lane;
            bool keep = false; double ac = 0.0, xc = 0.0;
            if (e < e1) {
                int j = jf; double gj = gf;
                if (eb != e0) { j = col[e]; gj = val[e]; }      // (rows of more than 64 entries: the later chunks as before)
                const unsigned char ii = isint[j];
                const double cl = gclo[j], ch = gchi[j], bl = h_lo[j], bh = h_hi[j];
                const double x = xs[j];
                if (ii) {
                    const double lo = bl, hi = bh;
                    if (lo == hi) rhs -= gj * lo;
                    else { const bool comp = x > 0.5; if (comp) rhs -= gj; keep = true; ac = comp ? -gj : gj; xc = comp ? 1.0 - x : x; }
                } else {
                    const double lo = cl, hi = ch;
                    const bool lof = lo > -0.5 * S_BIG, hif = hi < 0.5 * S_BIG;
                    if (gj > 0) { if (lof) rhs -= gj * lo; else if (hif) { rhs -= gj * hi; sval += gj * (hi - x); S2 += gj * gj; } else usable = 0; }
                    else { if (lof) { rhs -= gj * lo; sval += -gj * (x - lo); S2 += gj * gj; } else if (hif) rhs -= gj * hi; else usable = 0; }
                }
            }
            const unsigned long long bal = __ballot(keep);
            if (cnt + __popcll(bal) > cap) { usable = 0; over = true; break; }
            if (keep) { const int pos = cnt + __popcll(bal & ((1ull << lane) - 1ull)); ga[pos] = ac; gx[pos] = xc; }
            cnt += __popcll(bal);
        }
        rhs = wave_sum(rhs); sval = wave_sum(sval); S2 = wave_sum(S2);
        rhs = __shfl(rhs, 0, 64) + hsv; sval = __shfl(sval, 0, 64); S2 = __shfl(S2, 0, 64);
        int jn = 0; double gn = 0.0;
        if (has && e0n + lane < e1n) { jn = col[e0n + lane]; gn = val[e0n + lane]; }
        double best, bdelta;
#ifdef MLD_CUT_PROF
        const long long tp2 = wall_clock64();
        if (wave == 0 && lane == 0) sh.cprof[13] += tp2 - tp1;
#endif
        s_mir_score_row(ga, gx, cnt, lane, rhs, sval, S2, usable, split, sh, best, bdelta);
        if (lane == 0) { w.mir_eff[i] = best > 1e-4 ? best : -S_INF; w.mir_delta[i] = bdelta; }
#ifdef MLD_CUT_PROF
        if (wave == 0 && lane == 0) sh.cprof[14] += wall_clock64() - tp2;
#endif
        i = in; e0 = e0n; e1 = e1n; hsv = hsn; jf = jn; gf = gn;
    }
}

// column chunks a lane accumulates in registers per pass (n <= 576: one pass) and dictionary rows in flight together in the rows-outermost substitution
#define MIR_KC 9
#ifndef MIR_GROUP
#define MIR_GROUP 4
#endif
// phase B of s_mir_round, a wave per cut (see there).  L: every hot array of the pivot loop is in LDS as well as the lines -- LDS-typed views, and the
// substitution of the basic structurals with the rows outermost (below); L = false is round 4's code on generic pointers (MLD_DBG_CUTS_R4, other shapes).
template <bool L>
__device__ __forceinline__ int s_mir_build_waves(const Ws &w, Shared &sh, int max_cuts, int m_start, const lds_f64 *xs)
{
    const int n = w.n, ld = w.ld, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m0 = w.m0;
    HOT_VIEW(L, w);
    (void)h_dw; (void)h_d; (void)h_skip; (void)h_up;
    const typename CutT<L>::cu8p is_int = (typename CutT<L>::cu8p)w.is_int;
    const typename CutT<L>::u16p c_rowlist = (typename CutT<L>::u16p)w.rowlist, c_seclist = (typename CutT<L>::u16p)w.seclist;
    const typename HotT<L>::f64p c_colc = (typename HotT<L>::f64p)w.colc;
    const typename CutT<L>::cf64p clo = (typename CutT<L>::cf64p)w.clo, chi = (typename CutT<L>::cf64p)w.chi;
    const typename CutT<L>::gf64p mir_eff = (typename CutT<L>::gf64p)w.mir_eff, mir_delta = (typename CutT<L>::gf64p)w.mir_delta;
    int nc2 = 0;
    for (int i0 = 0; i0 < m0; i0 += SOL_NT) {
        const int i = i0 + tid;
        nc2 = block_compact(sh, i < m0 && mir_eff[i] > -S_INF, (unsigned short)i, w.rowlist, nc2);
    }
    __syncthreads();
    for (int t = tid; t < nc2; t += SOL_NT) c_colc[t] = mir_eff[c_rowlist[t]];
    __syncthreads();
    for (int t = tid; t < nc2; t += SOL_NT) {
        const int i = c_rowlist[t];
        const double e = c_colc[t];
        int rank = 0;
        for (int u = 0; u < nc2; ++u) { const double eu = c_colc[u]; rank += (eu > e) || (eu == e && (int)c_rowlist[u] < i); }
        c_seclist[rank] = (unsigned short)i;
    }
    __syncthreads();
    MLD_CHECK(w, nc2 <= m0 && nc2 <= (int)(w.rowlist - w.seclist), 121, nc2, m0);
    const typename HotT<L>::f64p axw = (typename HotT<L>::f64p)w.mir_cache + (size_t)wave * 2 * n;
    const typename CutT<L>::u16p rl = (typename CutT<L>::u16p)(axw + n);          // rows whose basic structural has a non-zero cut coefficient (at most n of them)
    int added = 0;
    for (int pos = 0; pos < nc2; pos += SOL_NW) {
        if (m_start + added >= sh.cut_cap || added >= max_cuts) break;
        const int t = pos + wave;
        bool ok = t < nc2;
        double bx = 0.0, nrm = 0.0, s_now = 0.0;
        if (ok) {
            const int i = c_seclist[t];
            const double delta = mir_delta[i];
            const typename CutT<L>::cf64p g = (typename CutT<L>::cf64p)(w.Gs + (size_t)i * n);
            const int jmax = w.nc_step > 0 ? min(n, (i / w.nc_step + 1) * w.nv_step) : n;      // causal rows (s_mir_phase_a)
            // right-hand side after complementing / bound substitution
            double rp = 0.0;
            for (int j = lane; j < jmax; j += 64) {
                const double gj = g[j];
                if (gj == 0.0) continue;
                if (is_int[j]) { const double lo = h_lo[j], hi = h_hi[j]; if (lo == hi) rp -= gj * lo; else if (xs[j] > 0.5) rp -= gj; }
                else { const double lo = clo[j], hi = chi[j]; rp -= gj * (lo > -0.5 * S_BIG ? lo : hi); }
            }
            const double rhs = wave_all_sum(rp) + ((typename CutT<L>::cf64p)w.hs)[i];
            const double b = rhs / delta, fb = floor(b), f = b - fb;
            ok = !(f < S_MIR_FMIN || f > 1.0 - S_MIR_FMIN);
            if (ok) {
                const double kc = 1.0 / (delta * (1.0 - f));
                double bp = 0.0, nm = 0.0;
                for (int j = lane; j < n; j += 64) {
                    double a = 0.0;
                    const double gj = j < jmax ? g[j] : 0.0;
                    if (gj != 0.0) {
                        if (is_int[j]) {
                            const double lo = h_lo[j], hi = h_hi[j];
                            if (lo != hi) {
                                const bool comp = xs[j] > 0.5;
                                const double aa = (comp ? -gj : gj) / delta, fl = floor(aa + 1e-12), fj = aa - fl;
                                const double cf = fl + (fj > f ? (fj - f) / (1.0 - f) : 0.0);
                                if (comp) { a = -cf; bp -= cf; } else a = cf;
                            }
                        } else {
                            const double lo = clo[j], hi = chi[j];
                            const bool lof = lo > -0.5 * S_BIG, hif = hi < 0.5 * S_BIG;
                            if (gj > 0) { if (!lof && hif) { a = kc * gj; bp += kc * gj * hi; } }
                            else { if (lof) { a = -kc * (-gj); bp -= kc * (-gj) * lo; } }
                        }
                    }
                    axw[j] = a;
                    nm = fmax(nm, fabs(a));
                }
                bx = fb + wave_all_sum(bp);
                nrm = wave_all_max(nm);
                ok = nrm > 0.0;
                if (ok) {
                    double sp = 0.0;
                    for (int j = lane; j < n; j += 64) { const double a = axw[j] / nrm; axw[j] = a; sp += a * xs[j]; }
                    s_now = bx / nrm - wave_all_sum(sp);
                    ok = s_now < -1e-9;               // not violated after all (rounding): skip
                }
            }
        }
        WAVE_MEM_SYNC();
        if (lane == 0) sh.s_i[wave] = ok ? 1 : 0;
        __syncthreads();
        int before = 0, total = 0;
        for (int u = 0; u < SOL_NW; ++u) { const int fl2 = sh.s_i[u]; if (u < wave) before += fl2; total += fl2; }
        const int room = min(sh.cut_cap - (m_start + added), max_cuts - added);
        if (ok && before < room) {
            const int kcut = m_start + added + before;
            MLD_CHECK(w, kcut >= m0 && kcut < w.mcap, 123, t, kcut);
            const typename CutT<L>::gf64p gk = (typename CutT<L>::gf64p)(w.Gc + (size_t)(kcut - m0) * n), dk = (typename CutT<L>::gf64p)(w.D + (size_t)kcut * ld);
            for (int j = lane; j < n; j += 64) gk[j] = axw[j];
            // dictionary row of the new slack: the cut row with the basic structurals substituted, dk = gk_N - sum_r gk[j_r] D[r,:] (rows of this round's
            // cuts have slack basics: only rows below m_start can qualify)
            int nbr = 0;
            for (int r0 = 0; r0 < m_start; r0 += 64) {
                const int r = r0 + lane;
                bool fl2 = false;
                if (r < m_start) { const int j = h_basic[r]; fl2 = j < n && axw[j] != 0.0; }
                const unsigned long long bal = __ballot(fl2);
                if (fl2) rl[nbr + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)r;
                nbr += __popcll(bal);
            }
            WAVE_MEM_SYNC();
            MLD_CHECK(w, nbr <= n && nbr <= m_start, 124, nbr, m_start);
            CUT_COUNT(sh, 6, 1); CUT_COUNT(sh, 7, nbr);
            const glb_f64 *Dg = (const glb_f64 *)w.D;
            double dp = 0.0;
            // Rows outermost when the coefficients fit behind rl in the wave's second line (n doubles: the nbr row indices take (nbr + 3) / 4 of them): the
            // coefficients axw[basic[rl[u]]] are gathered once, then MIR_GROUP rows at a time have ALL their column chunks in flight (MIR_GROUP x MIR_KC loads
            // per lane) before the chunks' accumulators are updated in ascending u -- per column the same acc -= cf_u * D[r_u, c] in the same order as the
            // round-4 nest (column chunk outermost, eight rows of one chunk in flight: MIR_KC x nbr / 8 dependent round trips per cut against nbr / MIR_GROUP),
            // and dp still adds up in ascending c per lane.
            bool rows_outer = false;
            if constexpr (L) rows_outer = (nbr + 3) / 4 + nbr <= n;
            if constexpr (L) if (rows_outer) {
                const typename HotT<L>::f64p cfl = (typename HotT<L>::f64p)(axw + n) + (nbr + 3) / 4;
                for (int u = lane; u < nbr; u += 64) cfl[u] = axw[h_basic[rl[u]]];
                WAVE_MEM_SYNC();
                for (int k0 = 0; k0 < n; k0 += 64 * MIR_KC) {
                    double acc[MIR_KC];
#pragma unroll
                    for (int q = 0; q < MIR_KC; ++q) {
                        const int c = k0 + q * 64 + lane;
                        acc[q] = 0.0;
                        if (c < n) { const int j = h_nonbasic[c]; acc[q] = j < n ? axw[j] : 0.0; }
                    }
                    for (int u = 0; u < nbr; u += MIR_GROUP) {
                        double v[MIR_GROUP][MIR_KC], cf[MIR_GROUP];
#pragma unroll
                        for (int e = 0; e < MIR_GROUP; ++e) {
                            const bool have = u + e < nbr;         // wave-uniform
                            const int r = __builtin_amdgcn_readfirstlane((int)rl[have ? u + e : u]);
                            const glb_f64 *row = Dg + (size_t)r * ld;
                            cf[e] = cfl[have ? u + e : u];
#pragma unroll
                            for (int q = 0; q < MIR_KC; ++q) { const int c = k0 + q * 64 + lane; v[e][q] = (have && c < n) ? row[c] : 0.0; }
                        }
#pragma unroll
                        for (int e = 0; e < MIR_GROUP; ++e) {
                            if (u + e >= nbr) continue;
#pragma unroll
                            for (int q = 0; q < MIR_KC; ++q) acc[q] -= cf[e] * v[e][q];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < MIR_KC; ++q) {
                        const int c = k0 + q * 64 + lane;
                        if (c < n) { dk[c] = acc[q]; dp += acc[q] * h_xN[c]; }
                    }
                }
            }
            if (!rows_outer)
            for (int c = lane; c < n; c += 64) {
                const int j = h_nonbasic[c];
                double acc = j < n ? axw[j] : 0.0;
                int u = 0;
                for (; u + 8 <= nbr; u += 8) {      // eight independent loads of the rows in flight
                    double v[8], cf[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) { const int r = rl[u + q]; v[q] = Dg[(size_t)r * ld + c]; cf[q] = axw[h_basic[r]]; }
#pragma unroll
                    for (int q = 0; q < 8; ++q) acc -= cf[q] * v[q];
                }
                for (; u < nbr; ++u) { const int r = rl[u]; acc -= axw[h_basic[r]] * Dg[(size_t)r * ld + c]; }
                dk[c] = acc;
                dp += acc * h_xN[c];
            }
            const double dsum = wave_all_sum(dp);
            if (lane == 0) {
                w.hc[kcut - m0] = bx / nrm;
                dk[n] = s_now + dsum;
                h_basic[kcut] = n + kcut; w.where[n + kcut] = -1 - kcut;
                h_xB[kcut] = s_now;
                h_lo[n + kcut] = 0.0; h_hi[n + kcut] = S_INF;
            }
        }
        added += min(total, room);
        __syncthreads();
    }
    return added;
}

__device__ int s_mir_round(const Ws &w, Shared &sh, int max_cuts)
{
    const int n = w.n, ld = w.ld, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m0 = w.m0;
    const int m_start = sh.m;
    lds_f64 *xs = (lds_f64 *)w.dabuf;
#ifdef MLD_CUT_PROF
    const long long tc_start = wall_clock64();
#endif
    __syncthreads();
    for (int c = tid; c < n; c += SOL_NT) { const int j = w.nonbasic[c]; if (j < n) xs[j] = w.xN[c]; }
    for (int r = tid; r < m_start; r += SOL_NT) { const int j = w.basic[r]; if (j < n) xs[j] = w.xB[r]; }
    __syncthreads();
    // ---- phase A: best (efficacy, delta) per original row.  Only rows that contain a fractional free binary can yield a cut:
    //      those binaries are listed first (ordered) and every row is pre-screened against the list with one load per lane.
    int nF = 0;
    for (int k0 = 0; k0 < w.nb; k0 += SOL_NT) {
        const int k = k0 + tid;
        bool fr = false; int j = 0;
        if (k < w.nb) { j = w.bins[k]; const double x = xs[j]; fr = w.lo[j] != w.hi[j] && x > 1e-6 && x < 1 - 1e-6; }
        nF = block_compact(sh, fr, (unsigned short)j, w.seclist, nF);
    }
    __syncthreads();
#ifdef MLD_CUT_PROF
    const long long tc_list = wall_clock64();
    if (tid == 0) sh.cprof[11] += tc_list - tc_start;
#endif
    // screen all rows at once (a thread per row, one load per listed binary): only rows that touch a fractional binary
    // are scored; they are compacted in row order and dealt to the waves
    int ncand = 0;
    if (w.csc_ptr && !(w.dbg & MLD_DBG_WALKS_SERIAL)) {
        // by columns: a thread per listed binary walks its column of the sparse copy and flags the rows it meets -- nF x 25 entries instead of one scattered
        // load per (live row, listed binary).  Both copies hold exactly the entries != 0.0 of the scaled rows, so a row is flagged if and only if the dense
        // screen below hits it.  The byte flags live in w.colc (8 mcap >= m0 bytes of LDS): the multiplier column of a pivot is dead between pivots, phase A
        // does not touch it and phase B overwrites it with its ranking keys after the barrier that ends phase A.
        const lds_u16 *fl = (const lds_u16 *)w.seclist;
        lds_u8 *rowflag = (lds_u8 *)w.colc;
        glb_ci32 *cp = (glb_ci32 *)w.csc_ptr; glb_cu16 *cr = (glb_cu16 *)w.csc_row;
        for (int i = tid; i < m0; i += SOL_NT) rowflag[i] = 0;
        __syncthreads();
        for (int k = tid; k < nF; k += SOL_NT) {
            const int j = fl[k];
            const int e0 = cp[j], e1 = cp[j + 1];
            for (int e = e0; e < e1; e += WALK_GROUP) {
                int ri[WALK_GROUP];
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) ri[q] = cr[min(e + q, e1 - 1)];      // (past the end: the last entry again)
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) { MLD_CHECK(w, ri[q] < m0, 143, ri[q], m0); rowflag[ri[q]] = 1; }      // (every writer stores the same value)
            }
        }
        __syncthreads();
        for (int i0 = 0; i0 < m0; i0 += SOL_NT) {
            const int i = i0 + tid;
            const bool hit = i < m0 && nF > 0 && !(w.skip[i] & 2) && rowflag[i] != 0;
            if (i < m0 && !hit) w.mir_eff[i] = -S_INF;
            ncand = block_compact(sh, hit, (unsigned short)i, w.rowlist, ncand);
        }
    } else {
        const lds_u16 *fl = (const lds_u16 *)w.seclist;
        for (int i0 = 0; i0 < m0; i0 += SOL_NT) {
            const int i = i0 + tid;
            bool hit = false;
            if (i < m0 && nF > 0 && !(w.skip[i] & 2)) {      // (a row that cannot bind under the bounds has no rounding that cuts a point inside them: s_mark_dead)
                const glb_f64 *g = (const glb_f64 *)(w.Gs + (size_t)i * n);
                for (int k0 = 0; k0 < nF; k0 += 8) {       // eight independent loads in flight
                    double gv[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) gv[q] = k0 + q < nF ? g[fl[k0 + q]] : 0.0;
#pragma unroll
                    for (int q = 0; q < 8; ++q) hit |= gv[q] != 0.0;
                }
            }
            if (i < m0 && !hit) w.mir_eff[i] = -S_INF;
            ncand = block_compact(sh, hit, (unsigned short)i, w.rowlist, ncand);
        }
    }
    __syncthreads();
#ifdef MLD_CUT_PROF
    if (tid == 0) sh.cprof[12] += wall_clock64() - tc_list;
#endif
    MLD_CHECK(w, nF <= w.nb && ncand <= m0, 120, nF, ncand);
    if (ncand > 0) {
        const bool split = w.mir_in_lds && !(w.dbg & MLD_DBG_CUTS_R4);       // several divisors of a row per wave (s_mir_score_sub)
        const bool pipe = w.csr_ptr && !(w.dbg & MLD_DBG_WALKS_SERIAL);      // the sparse copy exists: the pipelined pass 1 (s_mir_phase_a_pipe)
        lds_f64 *lga = w.mir_line ? (lds_f64 *)w.mir_line + (size_t)wave * 2 * w.mir_cap : (lds_f64 *)w.mir_cache + (size_t)wave * 2 * n;
        const int lcap = w.mir_line ? w.mir_cap : n;
        if (pipe && (w.mir_line || w.mir_in_lds) && w.all_lds) s_mir_phase_a_pipe<lds_f64 *, true>(lga, lga + lcap, lcap, w, xs, ncand, wave, lane, split, sh);
        else if (pipe && (w.mir_line || w.mir_in_lds)) s_mir_phase_a_pipe<lds_f64 *, false>(lga, lga + lcap, lcap, w, xs, ncand, wave, lane, split, sh);
        else if (pipe) s_mir_phase_a_pipe<double *, false>(w.mir_cache + (size_t)wave * 2 * n, w.mir_cache + (size_t)wave * 2 * n + n, n, w, xs, ncand, wave, lane, false, sh);
        else if (w.mir_line) s_mir_phase_a<lds_f64 *>((lds_f64 *)w.mir_line + (size_t)wave * 2 * w.mir_cap, (lds_f64 *)w.mir_line + (size_t)wave * 2 * w.mir_cap + w.mir_cap, w.mir_cap, w, xs, ncand, wave, lane, split, sh);
        else if (w.mir_in_lds) s_mir_phase_a<lds_f64 *>((lds_f64 *)w.mir_cache + (size_t)wave * 2 * n, (lds_f64 *)w.mir_cache + (size_t)wave * 2 * n + n, n, w, xs, ncand, wave, lane, split, sh);
        else s_mir_phase_a<double *>(w.mir_cache + (size_t)wave * 2 * n, w.mir_cache + (size_t)wave * 2 * n + n, n, w, xs, ncand, wave, lane, false, sh);
    }
    __syncthreads();
#ifdef MLD_CUT_PROF
    const long long tcA = wall_clock64();
    if (tid == 0) sh.cprof[0] += tcA - tc_start;
#endif
    // ---- phase B (round 4: a wave per cut, eight at a time; MLD_DBG_MIR_SERIAL keeps the one-at-a-time version for an A/B).  The candidates are ranked once
    //      by (efficacy descending, row ascending) -- the order the one-at-a-time loop takes them in; every wave builds the cut of its candidate with wave-level
    //      reductions only (the block-wide version spent eight barriers and reductions per cut: 11 % of the kernel), the accepted ones are appended in rank order.
    // While the per-wave lines fit LDS (cfg1-4 shapes).  At the cfg5 shape (n = 2303: lines in the slot, several hundred rows to substitute per cut) a wave per cut
    // measured 1.8 x SLOWER than the whole workgroup on one cut (15.5 s against 8.7 s for the 128 goldens): there the block-wide version below stays.
    if (!(w.dbg & MLD_DBG_MIR_SERIAL) && w.mir_in_lds) {
        const int added = (w.all_lds && !(w.dbg & MLD_DBG_CUTS_R4)) ? s_mir_build_waves<true>(w, sh, max_cuts, m_start, xs) : s_mir_build_waves<false>(w, sh, max_cuts, m_start, xs);
        __syncthreads();
        if (tid == 0) sh.m = m_start + added;
#ifdef MLD_CUT_PROF
        if (tid == 0) sh.cprof[1] += wall_clock64() - tcA;
#endif
        __syncthreads();
        return added;
    }
    // ---- phase B: the max_cuts most efficacious rows (smallest row index on ties), appended one by one
    int added = 0;
    for (;;) {
        __syncthreads();
        if (m_start + added >= sh.cut_cap || added >= max_cuts) break;
        double myv = -S_INF; int myi = -1;
        for (int i = tid; i < m0; i += SOL_NT) { const double e = w.mir_eff[i]; if (e > myv) { myv = e; myi = i; } }
        double bv;
        const int i = block_argmax(sh, myv, myi, &bv);
        if (i < 0 || bv == -S_INF) break;
        __syncthreads();
        const double delta = w.mir_delta[i];
        if (tid == 0) w.mir_eff[i] = -S_INF;
        const double *g = w.Gs + (size_t)i * n;
        // right-hand side after complementing / bound substitution
        double rp = 0.0;
        for (int j = tid; j < n; j += SOL_NT) {
            const double gj = g[j];
            if (gj == 0.0) continue;
            if (w.is_int[j]) { const double lo = w.lo[j], hi = w.hi[j]; if (lo == hi) rp -= gj * lo; else if (xs[j] > 0.5) rp -= gj; }
            else {
                const double lo = w.clo[j], hi = w.chi[j];
                const bool lof = lo > -0.5 * S_BIG, hif = hi < 0.5 * S_BIG;
                if (gj > 0) rp -= gj * (lof ? lo : hi); else rp -= gj * (lof ? lo : hi);
            }
        }
        const double rhs = block_sum(sh, rp) + w.hs[i];
        const double b = rhs / delta, fb = floor(b), f = b - fb;
        if (f < S_MIR_FMIN || f > 1.0 - S_MIR_FMIN) continue;
        const double kc = 1.0 / (delta * (1.0 - f));
        double bp = 0.0, nm = 0.0;
        for (int j = tid; j < n; j += SOL_NT) {
            const double gj = g[j];
            double a = 0.0;
            if (gj != 0.0) {
                if (w.is_int[j]) {
                    const double lo = w.lo[j], hi = w.hi[j];
                    if (lo != hi) {
                        const bool comp = xs[j] > 0.5;
                        const double aa = (comp ? -gj : gj) / delta, fl = floor(aa + 1e-12), fj = aa - fl;
                        const double cf = fl + (fj > f ? (fj - f) / (1.0 - f) : 0.0);
                        if (comp) { a = -cf; bp -= cf; } else a = cf;
                    }
                } else {
                    const double lo = w.clo[j], hi = w.chi[j];
                    const bool lof = lo > -0.5 * S_BIG, hif = hi < 0.5 * S_BIG;
                    if (gj > 0) { if (!lof && hif) { a = kc * gj; bp += kc * gj * hi; } }
                    else { if (lof) { a = -kc * (-gj); bp -= kc * (-gj) * lo; } }
                }
            }
            w.ax[j] = a;
            nm = fmax(nm, fabs(a));
        }
        const double bx = fb + block_sum(sh, bp);
        const double nrm = block_max(sh, nm);
        if (!(nrm > 0.0)) continue;
        const int kcut = m_start + added;
        MLD_CHECK(w, i >= 0 && i < m0 && kcut >= m0 && kcut < w.mcap, 123, i, kcut);
        double *gk = w.Gc + (size_t)(kcut - m0) * n, *dk = w.D + (size_t)kcut * ld;
        double sp = 0.0;
        for (int j = tid; j < n; j += SOL_NT) { const double a = w.ax[j] / nrm; w.ax[j] = a; gk[j] = a; sp += a * xs[j]; }
        const double s_now = bx / nrm - block_sum(sh, sp);
        if (!(s_now < -1e-9)) continue;               // not violated after all (rounding): skip
        // dictionary row of the new slack: the cut row with the basic structurals substituted, dk = gk_N - sum_r gk[j_r] D[r,:]
        int nbr = 0;
        for (int r0 = 0; r0 < m_start + added; r0 += SOL_NT) {
            const int r = r0 + tid;
            bool fl2 = false;
            if (r < m_start + added) { const int j = w.basic[r]; fl2 = j < n && w.ax[j] != 0.0; }
            nbr = block_compact(sh, fl2, (unsigned short)r, w.rowlist, nbr);
        }
        __syncthreads();
        MLD_CHECK(w, nbr <= m_start + added, 124, nbr, m_start + added);
        for (int t = tid; t < nbr; t += SOL_NT) w.colc[t] = w.ax[w.basic[w.rowlist[t]]];
        __syncthreads();
        double dp = 0.0;
        for (int c = tid; c < n; c += SOL_NT) {
            const int j = w.nonbasic[c];
            double acc = j < n ? w.ax[j] : 0.0;
            int t = 0;
            {   // the rows live in HBM and every load is a full latency: 16 of them in flight per thread
                const glb_f64 *Dg = (const glb_f64 *)w.D;
                const lds_u16 *rl = (const lds_u16 *)w.rowlist;
                const lds_f64 *cf = (const lds_f64 *)w.colc;
                for (; t + 16 <= nbr; t += 16) {
                    double v[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q) v[q] = Dg[(size_t)rl[t + q] * ld + c];
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc -= cf[t + q] * v[q];
                }
                for (; t + 4 <= nbr; t += 4) {
                    double v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = Dg[(size_t)rl[t + q] * ld + c];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc -= cf[t + q] * v[q];
                }
            }
            for (; t < nbr; ++t) acc -= w.colc[t] * w.D[(size_t)w.rowlist[t] * ld + c];
            dk[c] = acc;
            dp += acc * w.xN[c];
        }
        const double dsum = block_sum(sh, dp);
        if (tid == 0) {
            w.hc[kcut - m0] = bx / nrm;
            dk[n] = s_now + dsum;
            w.basic[kcut] = n + kcut; w.where[n + kcut] = -1 - kcut;
            w.xB[kcut] = s_now;
            w.lo[n + kcut] = 0.0; w.hi[n + kcut] = S_INF;
        }
        added++;
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) sh.m = m_start + added;
#ifdef MLD_CUT_PROF
    if (tid == 0) sh.cprof[1] += wall_clock64() - tcA;
#endif
    __syncthreads();
    return added;
}

__device__ void s_debug_dual(const Ws &w, Shared &sh, int inst, const char *where)
{   // debugging only: serial scan by thread 0
    __syncthreads();
    if (threadIdx.x == 0) {
        const double *d = w.dcost;
        int bad = 0, first = -1; double worst = 0;
        for (int c = 0; c < w.n; ++c) {
            const int j = w.nonbasic[c];
            if (w.lo[j] == w.hi[j]) continue;
            const double v = w.at_upper[c] ? d[c] : -d[c];
            if (v > 1e-7) { bad++; if (v > worst) { worst = v; first = c; } }
            const double bnd = w.at_upper[c] ? w.hi[j] : w.lo[j];
            if (w.xN[c] != bnd) MLD_PRINTF("[inst %d] %s: col %d var %d xN=%.6g not at bound %.6g (lo %.6g hi %.6g up %d)\n", inst, where, c, j, w.xN[c], bnd, w.lo[j], w.hi[j], (int)w.at_upper[c]);
            if (w.where[j] != c) MLD_PRINTF("[inst %d] %s: where[%d]=%d != col %d\n", inst, where, j, w.where[j], c);
        }
        if (bad) MLD_PRINTF("[inst %d] %s: %d dual infeasible columns, worst %.3e at col %d var %d (lo %.6g hi %.6g up %d d %.6g)\n", inst, where, bad, worst, first,
                        w.nonbasic[first], w.lo[w.nonbasic[first]], w.hi[w.nonbasic[first]], (int)w.at_upper[first], d[first]);
    }
    __syncthreads();
}

// Driebeek (1966) / Tomlin penalty branching (oracle/mld_oracle.c penalties()): for every fractional basic binary one dual ratio
// test on its dictionary row per side gives lower bounds pd / pu on the rise of the LP value in the down / up child.  A wave per
// candidate row (reduced costs and eligibility staged once in LDS); thread 0 then takes the oracle's sequential decision: the
// first candidate (binary index order) with one side lifted over the cutoff is branched with that side already closed, a
// candidate with both sides over the cutoff prunes the node, otherwise the largest product of penalties wins (first index on
// ties) and the side with the smaller penalty is explored first.
// Results: sh.s_i[0] branch variable (-1 none), s_i[1] first side (-1 = nearest), s_i[2] other side closed, s_i[3] node pruned,
// sh.s_d[1] smallest bound among the sides / nodes closed by the threshold only (t_next candidate, +inf if none).
__device__ void s_penalty_branch(const Ws &w, Shared &sh, const double *xs, double obj, double cut, double inc_cut)
{
    const int n = w.n, ld = w.ld, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    lds_u16 *cr = (lds_u16 *)w.rowlist, *cj = (lds_u16 *)w.seclist;
    lds_f64 *da = (lds_f64 *)w.dabuf, *pdl = (lds_f64 *)w.colc, *pul = (lds_f64 *)w.rowr;
    const glb_f64 *D = (const glb_f64 *)w.D;
    const double *d = w.dcost;
    __syncthreads();
    int C = 0;
    for (int k0 = 0; k0 < w.nb; k0 += SOL_NT) {
        const int k = k0 + tid;
        bool f = false; int j = 0, r = 0;
        if (k < w.nb) {
            j = w.bins[k];
            const double x = xs[j];
            if (fabs(x - rint(x)) > S_INTTOL && w.lo[j] != w.hi[j]) { const int wh = w.where[j]; if (wh < 0) { f = true; r = -1 - wh; } }      // (a FIXED binary is never a candidate, see the dive)
        }
        int rank;
        const int tot = block_rank(sh, f, &rank);
        if (f) { cr[C + rank] = (unsigned short)r; cj[C + rank] = (unsigned short)j; }
        C += tot;
    }
    for (int c = tid; c < n; c += SOL_NT) {
        const int j = w.nonbasic[c];
        da[c] = (w.lo[j] == w.hi[j]) ? -1.0 : fmax(w.at_upper[c] ? -d[c] : d[c], 0.0);
    }
    __syncthreads();
    MLD_CHECK(w, C <= w.nb && C <= w.mcap && C <= n, 126, C, w.nb);
    for (int t = wave; t < C; t += SOL_NW) {
        const int r = cr[t];
        MLD_CHECK(w, r >= 0 && r < sh.m, 127, t, r);
        const glb_f64 *row = D + (size_t)r * ld;
        double rd = S_INF, ru = S_INF;
        for (int c0 = 0; c0 < n; c0 += 512) {      // eight independent loads of the row in flight (one per iteration costs a memory latency each)
            double av[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) { const int c = c0 + q * 64 + lane; av[q] = c < n ? row[c] : 0.0; }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c = c0 + q * 64 + lane;
                if (c >= n) continue;
                const double a = av[q], dv = da[c];
                if (dv < 0.0 || fabs(a) <= 1e-9) continue;
                const double ratio = dv / fabs(a);
                if (w.at_upper[c] ? a < 0 : a > 0) rd = fmin(rd, ratio); else ru = fmin(ru, ratio);
            }
        }
        rd = wave_all_min(rd); ru = wave_all_min(ru);
        if (lane == 0) {
            const double xb = w.xB[r], f = xb - floor(xb);
            pdl[t] = rd < S_INF ? rd * f : S_INF;
            pul[t] = ru < S_INF ? ru * (1.0 - f) : S_INF;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const double eps = 1e-6 * fmax(1.0, fabs(obj));
        double bscore = -1.0, tn = S_INF;
        int bj = -1, ff = -1, sd = 0, pruned = 0, forced = 0;
        for (int t = 0; t < C; ++t) {
            const double pd = pdl[t], pu = pul[t];
            const bool xd = obj + pd > cut, xu = obj + pu > cut;
            if (xd && xu) {
                const double b = obj + fmin(pd, pu);
                pruned = 1; bj = -1;
                if (b <= inc_cut && b < tn) tn = b;
                break;
            }
            if (xd || xu) {
                const double b = obj + (xd ? pd : pu);
                if (b <= inc_cut && b < tn) tn = b;
                if (!forced) { forced = 1; bj = cj[t]; ff = xd ? 1 : 0; sd = 1; }
                continue;
            }
            if (forced) continue;
            const double sc = fmax(fmin(pd, 1e30), eps) * fmax(fmin(pu, 1e30), eps);
            if (sc > bscore) { bscore = sc; bj = cj[t]; ff = (pd == pu) ? -1 : (pd < pu ? 0 : 1); sd = 0; }
        }
        sh.s_i[0] = bj; sh.s_i[1] = ff; sh.s_i[2] = sd; sh.s_i[3] = pruned; sh.s_d[1] = tn;
    }
    __syncthreads();
}

// Evaluation of a complete binary assignment (a leaf of the search, or a MIP start -- oracle: leaf_eval): every free binary is fixed at the
// rounded entry of w.tmpx[], the remaining LP (QP) is solved on the same dictionary, the point is verified against the ORIGINAL rows and kept
// as the incumbent (best / have / v_out) when it is feasible and better; the bounds are restored.  Returns true when the rounded point is
// feasible.  All threads call; out of line (cold: once per leaf).
__device__ __noinline__ bool s_leaf_eval(const Ws &w, Shared &sh, const SolverShape &S, const double *plb, const double *pub, double *v_out,
                                         double &best, bool &have, bool &unbounded, int inst, int nodes)
{
    const int tid = threadIdx.x, n = S.n, nb = S.nb;
    const long long tl0 = wall_clock64();
    __syncthreads();
    if (tid == 0) {
        int ns = 0;
        if (w.dbg & MLD_DBG_WALKS_SERIAL)
        for (int k = 0; k < nb; ++k) {
            const int j = w.bins[k];
            if (w.lo[j] != w.hi[j]) { w.sv_j[ns] = j; w.sv_lo[ns] = w.lo[j]; w.sv_hi[ns] = w.hi[j]; w.key[ns] = fmin(fmax(rint(w.tmpx[j]), w.lo[j]), w.hi[j]); ns++; }
        }
        else {
            // the same list, one thread, WALK_GROUP binaries at a time: their indices, then bounds and values of all of them, then the entries in order (one
            // binary per iteration was two to three dependent round trips for each of the nb binaries, once per leaf)
            glb_ci32 *gb = (glb_ci32 *)w.bins; glb_cf64 *gx = (glb_cf64 *)w.tmpx;
            for (int k0 = 0; k0 < nb; k0 += WALK_GROUP) {
                int jj[WALK_GROUP]; double lo[WALK_GROUP], hi[WALK_GROUP], tx[WALK_GROUP];
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) jj[q] = gb[min(k0 + q, nb - 1)];
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q) { lo[q] = w.lo[jj[q]]; hi[q] = w.hi[jj[q]]; tx[q] = gx[jj[q]]; }
#pragma unroll
                for (int q = 0; q < WALK_GROUP; ++q)
                    if (k0 + q < nb && lo[q] != hi[q]) { w.sv_j[ns] = jj[q]; w.sv_lo[ns] = lo[q]; w.sv_hi[ns] = hi[q]; w.key[ns] = fmin(fmax(rint(tx[q]), lo[q]), hi[q]); ns++; }
            }
        }
        sh.s_i[0] = ns;
    }
    __syncthreads();
    const int ns = sh.s_i[0];
    MLD_CHECK(w, ns >= 0 && ns <= nb, 128, ns, nb);
    s_set_bounds_list(w, sh, w.sv_j, w.key, w.key, ns);
    const int lpl = s_dual_simplex(w, sh, S_INF, S.max_pivots);
    if ((S.debug & MLD_DBG_TRACE) && tid == 0) MLD_PRINTF("[inst %d] leaf lp=%d ns=%d node=%d\n", inst, lpl, ns, nodes);
    bool leaf_ok = (lpl == LP_OPTIMAL);
    if (leaf_ok && w.P) { double lbq, fvq; leaf_ok = s_sd_relax(w, sh, S_INF, S.max_pivots, &lbq, &fvq) == 0; }
    if (leaf_ok) {
        if (w.P) { __syncthreads(); for (int j = tid; j < n; j += SOL_NT) w.xo[j] = w.vcur[j]; __syncthreads(); }
        else s_gather_x(w, sh, w.xo);
        for (int k = tid; k < nb; k += SOL_NT) { const int j = w.bins[k]; w.xo[j] = rint(w.xo[j]); }
        __syncthreads();
        double part = 0.0;
        for (int j = tid; j < n; j += SOL_NT) part += w.qs[j] * w.xo[j];
        double ob = block_sum(sh, part);
        if (w.P) { s_matvecP(w, w.xo, w.Pv); ob += 0.5 * s_dot(sh, w.xo, w.Pv, n); }
        // feasibility against the original (scaled) rows
        double worst = -S_INF;
        {
            const int wave = tid >> 6, lane = tid & 63;
            lds_f64 *xs = (lds_f64 *)w.dabuf;
            const glb_f64 *Gg = (const glb_f64 *)w.Gs;
            __syncthreads();
            for (int j = tid; j < n; j += SOL_NT) xs[j] = w.xo[j];
            __syncthreads();
            if (w.csr_ptr) {      // (the sparse copy of the rows, a thread per row: s_check_residual)
                for (int i = tid; i < S.m0; i += SOL_NT) {
                    double acc = 0.0;
                    const int e1 = w.csr_ptr[i + 1];
                    if (w.dbg & MLD_DBG_WALKS_SERIAL) { for (int e = w.csr_ptr[i]; e < e1; ++e) acc += w.csr_val[e] * xs[w.csr_col[e]]; }
                    else {
                        glb_cu16 *rc = (glb_cu16 *)w.csr_col; glb_cf64 *rv = (glb_cf64 *)w.csr_val;
                        for (int e = w.csr_ptr[i]; e < e1; e += WALK_GROUP) {
                            int cj[WALK_GROUP]; double cg[WALK_GROUP], xv[WALK_GROUP];
#pragma unroll
                            for (int q = 0; q < WALK_GROUP; ++q) { const int eq = min(e + q, e1 - 1); cj[q] = rc[eq]; cg[q] = rv[eq]; }
#pragma unroll
                            for (int q = 0; q < WALK_GROUP; ++q) xv[q] = xs[cj[q]];
#pragma unroll
                            for (int q = 0; q < WALK_GROUP; ++q) if (e + q < e1) acc += cg[q] * xv[q];
                        }
                    }
                    worst = fmax(worst, acc - w.hs[i]);
                }
            } else
            for (int i0 = wave * 4; i0 < S.m0; i0 += SOL_NW * 4) {
                const glb_f64 *rp[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) rp[q] = Gg + (size_t)(i0 + q < S.m0 ? i0 + q : i0) * n;
                double sv[4];
                wave_rows_dot4(rp[0], rp[1], rp[2], rp[3], xs, n, lane, sv, (w.dbg & MLD_DBG_WALKS_SERIAL) != 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double t = wave_sum(sv[q]);
                    if (lane == 0 && i0 + q < S.m0) worst = fmax(worst, t - w.hs[i0 + q]);
                }
            }
        }
        worst = block_max(sh, worst);
        if ((S.debug & MLD_DBG_TRACE) && tid == 0) MLD_PRINTF("[inst %d] leaf ob=%.12g worst=%.3e best=%.12g node=%d\n", inst, ob, worst, best, nodes);
        if (worst <= 1e-6 && ob < best) {
            best = ob; have = true;
            for (int j = tid; j < n; j += SOL_NT) v_out[j] = w.xo[j] * w.cs[j];
        }
        if (worst <= 1e-6) {
            // A free variable resting NON-BASIC on the artificial box (+-S_BIG) with a non-zero reduced cost: no finite
            // optimum.  With a zero reduced cost the box is only where a variable the objective does not depend on happens
            // to sit (oracle: same rule).  QP relaxations keep the plain test on the point.
            double hit = 0.0;
            if (w.P) {
                for (int j = tid; j < n; j += SOL_NT)
                    if ((plb[j] == -S_INF && w.xo[j] <= -0.999 * S_BIG) || (pub[j] == S_INF && w.xo[j] >= 0.999 * S_BIG)) hit = 1.0;
            } else {
                const double *dd = w.dcost;
                for (int c = tid; c < n; c += SOL_NT) {
                    const int j = w.nonbasic[c];
                    if (j >= n || fabs(dd[c]) <= 1e-9) continue;
                    if ((plb[j] == -S_INF && w.xN[c] <= -0.999 * S_BIG) || (pub[j] == S_INF && w.xN[c] >= 0.999 * S_BIG)) hit = 1.0;
                }
            }
            if (block_max(sh, hit) > 0.0) unbounded = true;
        }
        leaf_ok = worst <= 1e-6;
    }
    s_set_bounds_list(w, sh, w.sv_j, w.sv_lo, w.sv_hi, ns);
    if (tid == 0) sh.prof[3] += wall_clock64() - tl0;
    __syncthreads();
    return leaf_ok;
}


// In-kernel hand-off: publish open nodes of the calling search as queue entries (items).  The stack holds `depth` levels; a level whose sibling has
// not been visited (stk_second == 0) stands for the open node {path above it, that level flipped}.  take_all: every such level plus the current path
// itself (the search stops); otherwise the `kmax` SHALLOWEST such levels -- the largest open subtrees -- which are then marked as accounted for (the
// search goes on below them).  Returns the number of items published (0: nothing to publish, no room, or the tree has been given up).  All threads call.
__device__ __noinline__ int s_publish_nodes(const Ws &w, Shared &sh, const ProblemDev &P, const BatchDev &B, int nb, int inst, int isrc, bool is_item,
                                            const unsigned char *fixed, int depth, bool take_all, int kmax, double cut_child, const unsigned char *pval, bool include_current)
{   // pval: the levels' current values (null: read them off the bounds); include_current: the current path itself is an open node (take_all only).
    // Returns the number of items published, 0 when nothing is open (the search is closed), -1 when they could not be published.
    const int tid = threadIdx.x;
    const int gen = is_item ? B.item_gen[inst] : 0;
    __syncthreads();
    if (tid == 0) {
        int nc = (take_all && include_current) ? 1 : 0;
        for (int k = 0; k < depth; ++k) if (!w.stk_second[k] && (take_all || nc < kmax)) nc++;
        int base = -1;
        const int root_t = is_item ? B.item_root[inst] : inst;
        bool room_tree = nc > 0 && gen < B.ho_max_gen && nc <= B.ho_max_children && B.item_children[inst] + nc <= 128;      // (tree labels: 128 children per entry)
        // (the host-driven hand-off's rule, round for round: a tree whose open nodes of ONE generation outnumber the cap keeps growing -- it is given up)
        if (room_tree && __hip_atomic_fetch_add(&B.tree_count[(size_t)root_t * 9 + gen], nc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + nc > B.ho_max_tree) {
            __hip_atomic_store(&B.tree_dead[root_t], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // too many open nodes: the tree is given up
            room_tree = false;
        }
        if (room_tree) {
            int old = __hip_atomic_load(B.tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (old + nc <= B.cap) {
                if (__hip_atomic_compare_exchange_strong(B.tail, &old, old + nc, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { base = old; break; }
            }
            if (base < 0) __hip_atomic_store(&B.tree_dead[root_t], 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (no room in the queue: given up as well -- the one case that depends on the order; counted)
        }
        sh.s_i[5] = base; sh.s_i[6] = nc;
    }
    __syncthreads();
    const int base = sh.s_i[5], nc = sh.s_i[6];
    if (nc == 0) return 0;
    if (base < 0) return -1;
    unsigned char *path = (unsigned char *)w.key;           // (free here: nb bytes of the slot)
    for (int b = tid; b < nb; b += SOL_NT) path[b] = fixed ? fixed[b] : (unsigned char)255;
    __syncthreads();
    int c = 0;
    for (int k = 0; k < depth && (take_all || c < nc); ++k) {
        const int j = w.stk_j[k], pb = P.binpos[j];
        const unsigned char val = pval ? pval[k] : (unsigned char)(w.lo[j] > 0.5 ? 1 : 0);
        MLD_CHECK(w, pb >= 0 && pb < nb && base + c < B.cap, 140, j, pb);
        const bool open_k = !w.stk_second[k];
        __syncthreads();
        if (open_k) {
            unsigned char *dst = B.fixed + (size_t)(base + c) * nb;
            for (int b = tid; b < nb; b += SOL_NT) dst[b] = (b == pb) ? (unsigned char)(1 - val) : path[b];
            if (!take_all && tid == 0) w.stk_second[k] = 1;      // handed off: the search does not come back to this sibling
            c++;
        }
        __syncthreads();
        if (tid == 0) path[pb] = val;
        __syncthreads();
    }
    if (take_all && include_current) {
        unsigned char *dst = B.fixed + (size_t)(base + c) * nb;
        for (int b = tid; b < nb; b += SOL_NT) dst[b] = path[b];
    }
    const int root = is_item ? B.item_root[inst] : inst;
    const long long label = is_item ? B.item_label[inst] : 1ll;
    const int first_child = B.item_children[inst];            // (labels stay distinct when a search publishes more than once)
    for (int c2 = tid; c2 < nc; c2 += SOL_NT) {
        const int it = base + c2;
        B.item_src[it] = isrc; B.item_root[it] = root; B.item_gen[it] = gen + 1; B.item_label[it] = label * 129 + (first_child + c2) + 1;
        B.cutoff[it] = cut_child; B.item_children[it] = 0;
        if (B.open_depth) B.open_depth[it] = -1;
    }
    __threadfence();                                     // every thread's part of the items is visible device-wide ...
    __syncthreads();
    for (int c2 = tid; c2 < nc; c2 += SOL_NT) __hip_atomic_store(&B.item_ready[base + c2], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);   // ... before any of them can be claimed
    if (tid == 0) B.item_children[inst] = first_child + nc;
    __syncthreads();
    return nc;
}

__device__ __forceinline__ double s_gtol(const SolverShape &S, double v) { return fmax(S.gap_abs, S.gap_rel * fabs(v)); }

// one round of cut separation (Gomory, then rounding cuts): called from the root cut loop and from the root restart -- one copy of the code
__device__ __noinline__ int s_cut_round(const Ws &w, Shared &sh, const SolverShape &S)
{
#ifdef MLD_CUT_PROF
    const long long t0 = wall_clock64();
#endif
    int k = (S.debug & MLD_DBG_GMI_SERIAL) ? s_gmi_round_serial(w, sh, S.cuts_per_round) : s_gmi_round(w, sh, S.cuts_per_round);
#ifdef MLD_CUT_PROF
    if (threadIdx.x == 0) { sh.cprof[2] += wall_clock64() - t0; sh.cprof[3] += 1; }
#endif
    if (S.mir_per_round > 0) k += s_mir_round(w, sh, S.mir_per_round);
    return k;
}

// ------------------------------------------------------------------------------------------------
// the persistent solve kernel: a claim loop over queue entries, each solved in inlined stages (a call on the node path costs the callee-saved
// spills of a 256-VGPR function, DESIGN section 6): s_setup_entry, s_root, s_search, s_write_results
// ------------------------------------------------------------------------------------------------
// One queue entry, an instance or an item of the in-kernel hand-off (an open node of another search); read-only once set up.  inst: output row (an item's
// can exceed a SUB-batch's size: the overflow list of the LDS paths holds instance numbers); isrc: the instance whose inputs (x0, omega, right-hand side,
// model mdl) it uses; ext_cut: an external cutoff (hand-off: the value of the incumbent the open node was cut out of) -- the search looks only for better
// points; fixed / warm: fixed binaries (255: free) / MIP start, or null; r_const: c0 + cx.x0 + cw.w (+ quadratic constant; controller_base.py:533-538)
struct Entry {
    int inst, isrc, mdl, max_nodes;
    bool is_item, ext_cut;
    const unsigned char *fixed, *warm;
    const double *plb, *pub;
    double *v_out, r_const;
    long long t_begin;
};

// What the entry's solve has found and proven so far: the write-out reports it.
struct Search {
    double best = S_INF, root_bound = -S_INF, lb_proven = -S_INF;
    int status = MLD_STATUS_INFEASIBLE, nodes = 1, cuts = 0;
    bool have = false, unbounded = false;
};

// The search: iterative-deepening depth-first branch-and-bound, with a look-ahead dive and RINS for the degenerate instances (phases: see
// oracle/mld_oracle.c, orc_solve_miqp).  Tree: the state of the phase loop and of its current pass; Node: what the node just evaluated leaves to decide.
enum { PH_IDS = 0, PH_DIVE, PH_RINS, PH_FINAL };
struct Tree {
    int phase, pass = 0, node_budget, ids_cap, rins_rounds = 0, nfix = 0, donations = 0, lp = LP_OPTIMAL;      // lp: status of the last node's LP
    double T, lbg, restart_best = S_INF, dive_tol;      // T: threshold of the passes; lbg: proven global lower bound (raised by every exhaustive pass)
    bool limit = false, rescue = false, timed_out = false, started = false, xroot_set = false;
    bool expanded = false, stopped_complete = false, published_rest = false;      // in-kernel hand-off: items published / the stopped search / all of its rest
    int depth; double t_next, best_at_start; bool finished, dive_end;      // the current pass
    // a COMPLETE search (plain depth-first search below the incumbent: FINAL, or the deepening passes once T is infinite) stopped at a limit: the stack
    // describes everything that is still open -- for every level whose sibling has not been visited the node (path above it, variable flipped), plus the current path
    __device__ bool complete() const { return limit && !finished && !rescue && (phase == PH_FINAL || (phase == PH_IDS && T == S_INF)); }
};
struct Node {
    int branch_j = -1, force_first = -1; double branch_x = 0.0, obj = S_INF;
    bool second_done = false, pen_pruned = false;      // penalty branching: preferred side, other side closed
    bool qp_open = false;      // (quadratic cost: the node's QP relaxation hit the limit -- the node is unsolved, still open)
};
// s_leaf_eval on the entry's incumbent (through locals: a member of Search whose address reached the call would keep all of Search in scratch)
__device__ __forceinline__ bool s_leaf(const Ws &w, Shared &sh, const SolverShape &S, const Entry &e, Search &s, int nodes)
{
    double best = s.best; bool have = s.have, unbounded = s.unbounded;
    const bool ok = s_leaf_eval(w, sh, S, e.plb, e.pub, e.v_out, best, have, unbounded, e.inst, nodes);
    s.best = best; s.have = have; s.unbounded = unbounded;
    return ok;
}

// Entry set-up: the entry's model and inputs, the bounds with its fixings, its objective constant and cutoff, the per-instance presolve and the
// rows that cannot bind.  Returns false when the presolve finds no point that satisfies the rows under the bounds (nothing to solve).
__device__ __forceinline__ bool s_setup_entry(Ws &w, Shared &sh, const SolverShape &S, const ProblemDev &P, const BatchDev &B, Entry &e, Search &s)
{
    const int tid = threadIdx.x, n = S.n, nb = S.nb, inst = e.inst, isrc = e.isrc;
    const int mdl = e.mdl = B.model_idx ? B.model_idx[isrc] : 0;
    w.Gs = P.Gs + (size_t)mdl * S.m0 * n; w.hs = B.hs + (size_t)isrc * S.m0;
    w.Gp = P.Gp ? P.Gp + (size_t)mdl * S.m0 * n : nullptr;
    w.csr_ptr = P.csr_ptr ? P.csr_ptr + (size_t)mdl * (S.m0 + 1) : nullptr; w.csr_col = P.csr_ptr ? P.csr_col + (size_t)mdl * P.nnz_cap : nullptr; w.csr_val = P.csr_ptr ? P.csr_val + (size_t)mdl * P.nnz_cap : nullptr;
    w.csc_ptr = (P.csr_ptr && P.csc_ptr) ? P.csc_ptr + (size_t)mdl * (n + 1) : nullptr; w.csc_row = w.csc_ptr ? P.csc_row + (size_t)mdl * P.nnz_cap : nullptr;
    w.qs = B.qs_inst ? B.qs_inst + (size_t)isrc * n : P.qs + (size_t)mdl * n; w.cs = P.cs + (size_t)mdl * n;
    w.P = (S.qp && P.Ps) ? P.Ps + (size_t)mdl * n * n : nullptr;
    w.is_int = P.is_int; w.bins = P.bins; w.colperm = P.colperm;
    e.plb = P.lb + (size_t)mdl * n; e.pub = P.ub + (size_t)mdl * n;
    e.fixed = (B.fixed && (e.is_item || !(B.ho & 2))) ? B.fixed + (size_t)inst * nb : nullptr;      // (ho bit 1: the caller uploaded no fixings -- only items have them)
    e.warm = (!e.is_item && B.warm && nb > 0 && B.warm[(size_t)inst * nb] != 255) ? B.warm + (size_t)inst * nb : nullptr;
    e.v_out = B.v_out + (size_t)inst * n;
    e.t_begin = wall_clock64();
    if (tid == 0) { sh.m = S.m0; sh.pivots = 0; sh.refactors = 0; sh.since_check = 0; sh.rows = 0ull; sh.perturbed = 0; sh.bfrt = 0; for (int k = 0; k < 8; ++k) sh.prof[k] = 0;
        sh.cut_cap = S.first_cap;
        sh.deadline = 0; sh.timed_out = 0;      // (armed when the search starts: the root LP always runs to its end -- without it there is no answer at all)
#ifdef MLD_PIVOT_PROF
        for (int k = 0; k < 8; ++k) sh.pprof[k] = sh.pcnt[k] = 0;
        for (int k = 0; k < 9; ++k) sh.sprof[k] = 0;
#endif
#ifdef MLD_CUT_PROF
        for (int k = 0; k < 15; ++k) sh.cprof[k] = 0;
#endif
    }
    for (int j = tid; j < n; j += SOL_NT) { w.lo[j] = e.plb[j]; w.hi[j] = e.pub[j]; e.v_out[j] = 0.0; }
    for (int i = tid; i < S.mcap; i += SOL_NT) { w.lo[n + i] = 0.0; w.hi[n + i] = S_INF; }
    __syncthreads();
    if (e.fixed)
        for (int k = tid; k < nb; k += SOL_NT) if (e.fixed[k] != 255) { const int j = w.bins[k]; w.lo[j] = w.hi[j] = (double)e.fixed[k]; }
    __syncthreads();
    double part = 0.0;
    if (P.cx) for (int j = tid; j < S.nx; j += SOL_NT) part += P.cx[(size_t)mdl * S.nx + j] * B.x0[(size_t)isrc * S.nx + j];
    if (P.cw) for (int j = tid; j < S.nW; j += SOL_NT) part += P.cw[(size_t)mdl * S.nW + j] * B.omega[(size_t)isrc * S.nW + j];
    e.r_const = block_sum(sh, part) + (P.c0 ? P.c0[mdl] : 0.0) + (B.rconst ? B.rconst[isrc] : 0.0);
    e.ext_cut = B.cutoff && B.cutoff[inst] < 1.0e300;
    if (e.ext_cut) s.best = B.cutoff[inst] - e.r_const;
    if (tid == 0 && B.open_depth) B.open_depth[inst] = -1;
    for (int j = tid; j < n; j += SOL_NT) { w.clo[j] = w.lo[j]; w.chi[j] = w.hi[j]; }
    const bool pre_on = S.presolve && P.csr_ptr && !(S.debug & MLD_DBG_NO_PRESOLVE);
    const bool pre_ok = !pre_on || s_presolve(w, sh, P, mdl);
    if (!pre_ok && e.ext_cut) s.lb_proven = s.best - s_gtol(S, s.best) + 1e-12;      // (status: infeasible)
    s_mark_dead(w, sh, !(S.debug & MLD_DBG_KEEP_DEAD_ROWS), (!e.fixed && P.act_max) ? P.act_max + (size_t)mdl * S.m0 : nullptr, (pre_on && pre_ok) ? &P : nullptr, mdl);
    // (round 4: also under a quadratic cost -- a row that cannot bind under the root bounds cannot block a primal ratio test either, and s_primal_simplex skips such rows)
    return pre_ok;
}

// Cut rows whose slack still sits basic in its own row (the cut never had to leave) and is clearly positive when a cut loop ends are not maintained
// below the root (oracle: same rule): dropping a cut is always valid, the rank-1 updates skip the row (measured on the bench shard: 9.5 % fewer row
// updates, 3.8 % less kernel time, proven share unchanged)
__device__ __forceinline__ void s_purge_slack_cuts(const Ws &w, Shared &sh)
{
    __syncthreads(); for (int i = w.m0 + threadIdx.x; i < sh.m; i += SOL_NT) if (w.basic[i] == w.n + i && w.xB[i] > S_PURGE_SLACK) w.skip[i] = 2; __syncthreads();
}

// Cut rounds at an optimal root LP, each re-solved under `cutoff`: they end when a round finds no cut, after `rounds` rounds, after `patience` rounds
// without progress of the bound, or at an LP that is not optimal (its status is returned).  The root cut loop (root_loop) also ends when an eager
// start's incumbent is within the gap of the bound and at the TimeLimit; the root restart ends when the cut rows are full.
__device__ __forceinline__ int s_cut_loop(const Ws &w, Shared &sh, const SolverShape &S, const Entry &e, Search &s, double cutoff, int rounds, int patience, bool root_loop)
{
    const int tid = threadIdx.x;
    int stalled = 0;
    for (int rnd = 0; rnd < rounds; ++rnd) {
        if (!root_loop && sh.m >= S.mcap) break;
        const double before = s_objective(w, sh);
        const long long tc0 = wall_clock64();
        if (root_loop) MLD_MARK(w, sh, 10 + rnd);
        const int k = s_cut_round(w, sh, S);
        if (tid == 0) sh.prof[2] += wall_clock64() - tc0;
        if (root_loop) MLD_MARK(w, sh, 50 + rnd);
        if (!k) break;
        s.cuts += k;
        const int cap = sh.pivots + 4 * S.m0 + 200;          // a cut round never needs more than this
        const int lp = s_dual_simplex(w, sh, cutoff, cap < S.max_pivots ? cap : S.max_pivots);
        if (lp != LP_OPTIMAL) return lp;
        const double after = s_objective(w, sh);
        if (root_loop && s.have && !e.ext_cut && after >= s.best - s_gtol(S, s.best)) break;      // (eager start: the bound is within the gap of the incumbent -- nothing left to prove)
        if (after - before < 1e-6 * fmax(1.0, fabs(before))) { if (++stalled >= patience) break; } else stalled = 0;
        if (root_loop && S.time_ticks > 0) {      // TimeLimit between cut rounds: the loop ends, the search takes the rest of the verdict
            __syncthreads(); if (tid == 0) sh.timed_out = wall_clock64() - e.t_begin > S.time_ticks ? 1 : 0; __syncthreads();
            if (sh.timed_out) break;
        }
    }
    return LP_OPTIMAL;
}

// The root: LP + cut rounds.  If the LP breaks down while cutting (iteration cap / false infeasibility on a highly degenerate face), the root is rebuilt
// from scratch and solved without cuts.  Under a quadratic cost the QP relaxation then gives the root bound.  Returns whether the search can start.
__device__ __forceinline__ bool s_root(const Ws &w, Shared &sh, const SolverShape &S, const Entry &e, Search &s)
{
    const int tid = threadIdx.x, n = S.n, nb = S.nb;
    bool root_ok = false, eager_done = false;
    for (int attempt = 0; attempt < 2 && !root_ok; ++attempt) {
        const bool use_cuts = (attempt == 0) && S.cut_rounds > 0;
        __syncthreads(); if (tid == 0) sh.m = S.m0; __syncthreads();
        s_reset_dictionary(w, sh);
        for (int c = tid; c < n; c += SOL_NT) {   // place every non-basic at its dual-feasible bound
            const int j = w.nonbasic[c];
            const double dc = w.qs[j];
            double lo = w.lo[j], hi = w.hi[j];
            if (lo == hi) { w.at_upper[c] = 0; w.xN[c] = lo; }
            else if (dc >= 0) { if (lo == -S_INF) { lo = -S_BIG; w.lo[j] = lo; } w.at_upper[c] = 0; w.xN[c] = lo; }
            else { if (hi == S_INF) { hi = S_BIG; w.hi[j] = hi; } w.at_upper[c] = 1; w.xN[c] = hi; }
        }
        if (w.csr_ptr && sh.m == S.m0) s_refresh_initial(w, sh); else s_refresh(w, sh);
        if (tid == 0 && attempt == 0) sh.prof[6] += wall_clock64() - e.t_begin;
        __syncthreads();
        MLD_MARK(w, sh, 2 + 1000 * attempt);
        if (e.warm && !eager_done && !(S.debug & MLD_DBG_LAZY_START) && !w.P) {
            // The MIP start FIRST (round 4; round 3 evaluated it lazily, only when the deepening passes ended without an incumbent -- MLD_DBG_LAZY_START
            // restores that for an A/B): its leaf LP from the slack basis -- every binary fixed, an easy LP --, then the root relaxation from
            // the leaf's basis.  In a closed loop the shifted plan is near-optimal, so the relaxation's optimum is a few pivots away from the leaf's
            // vertex, the incumbent is known before the first cut, and the cut loop stops as soon as the bound is within the gap of it: closed loop
            // step 24 7.5 k/s instead of 5.4 k/s (pivots per instance 340 instead of 434), step 4 27 k/s instead of 21 k/s, proven share unchanged
            eager_done = true;
            __syncthreads(); for (int k = tid; k < nb; k += SOL_NT) w.tmpx[w.bins[k]] = (double)e.warm[k]; __syncthreads();
            (void)s_leaf(w, sh, S, e, s, 0);      // (a leaf, not a node of the tree: not counted)
        }
        if (tid == 0) sh.bfrt = (!w.P && !(S.debug & MLD_DBG_NO_LONG_STEP)) ? 1 : 0;      // long-step ratio test: root LP only
        __syncthreads();
        // Under an external cutoff (an open node handed off by another search) the root LP and every cut round stop as soon as the bound passes the
        // cutoff: "nothing better in this node" is then known for a fraction of a root LP (83 % of the items of a bench shard end exactly so).
        const double root_cut = e.ext_cut ? s.best - s_gtol(S, s.best) + 1e-12 : S_INF;
        int lp = s_dual_simplex(w, sh, root_cut, S.max_pivots);
        __syncthreads(); if (tid == 0) sh.bfrt = 0; __syncthreads();
        if (lp == LP_CUTOFF) { s.status = MLD_STATUS_INFEASIBLE; s.lb_proven = root_cut; break; }
        if (lp != LP_OPTIMAL) { s.status = (lp == LP_INFEASIBLE) ? MLD_STATUS_INFEASIBLE : MLD_STATUS_NUMERICAL; break; }
        root_ok = true;
        s.cuts = 0;
        if (use_cuts) {
            lp = s_cut_loop(w, sh, S, e, s, root_cut, S.cut_rounds, S_CUT_PATIENCE, true);
            MLD_MARK(w, sh, 70);
            if (lp == LP_CUTOFF) { s.status = MLD_STATUS_INFEASIBLE; s.lb_proven = root_cut; root_ok = false; break; }     // (external cutoff: the node is closed by its bound)
            if (lp != LP_OPTIMAL) { root_ok = false; s.status = MLD_STATUS_NUMERICAL; s.cuts = 0; }       // rebuild without cuts
            else s_purge_slack_cuts(w, sh);
        }
    }
    if (root_ok && w.P) {   // root bound of the QP relaxation
        // (an item of the in-kernel hand-off stops as soon as the bound passes its cutoff, as its root LP does: "nothing better in this node")
        const double qcut = (e.is_item && e.ext_cut) ? s.best - s_gtol(S, s.best) + 1e-12 : S_INF;
        double lbq, fvq;
        const int rcq = s_sd_relax(w, sh, qcut, S.max_pivots, &lbq, &fvq);
        if (rcq == 1) { root_ok = false; s.status = MLD_STATUS_INFEASIBLE; s.lb_proven = qcut; }
        else if (rcq == -1) { root_ok = false; s.status = MLD_STATUS_NUMERICAL; }
        else s.root_bound = rcq == -2 ? s_objective(w, sh) : lbq;      // (-2: the QP relaxation could not be finished -- the LP(q) value is a bound too)
    }
    if (root_ok && !w.P) s.root_bound = s_objective(w, sh);
    return root_ok;
}

// Root restart (round 4; oracle: same rule; MLD_DBG_NO_RESTART switches it off for an A/B).  The final search is about to start from the root with
// an incumbent that is CLOSE to the proven bound but not within the gap -- under the flat mid-day tariff that is the whole unproven tail (reported
// gaps: median 1.7 %).  More cut rounds at the root, now under the incumbent's cutoff and in the cut rows the root cut loop left free, move the
// bound the last percent for most of them (256 flat-tariff bench instances on the CPU restatement: 3 -> 1 unproven, -3 % row updates; instances
// that never get here are untouched).  The cut loop itself may not be longer: ten rounds are what pays on the whole shard (DESIGN section 9).
// Not for an instance with a MIP start: its cut loop already ran against the start's value (it ends when the bound is within the gap of it), and
// in the closed loop the restart cost 8 % of the steady-state step for one more proven instance in 10 000.
// Returns true when the root is closed by its bound under the incumbent's cutoff: nothing better than the incumbent by more than the gap exists.
__device__ __forceinline__ bool s_root_restart(const Ws &w, Shared &sh, const SolverShape &S, const Entry &e, Search &s, Tree &t)
{
    if (!(t.phase == PH_FINAL && s.have && !e.warm && !e.ext_cut && !t.rescue && !w.P && S.cut_rounds > 0 && sh.m < S.mcap && s.best < t.restart_best &&
          s.best - t.lbg <= S_RESTART_GAPS * s_gtol(S, s.best) && s.nodes >= e.max_nodes / 8 && !(S.debug & MLD_DBG_NO_RESTART)))
        return false;
    t.restart_best = s.best;
    const double rcut = s.best - s_gtol(S, s.best) + 1e-12;
    __syncthreads(); if (threadIdx.x == 0) sh.cut_cap = S.mcap; __syncthreads();
    MLD_MARK(w, sh, 90);
    int lp = s_dual_simplex(w, sh, rcut, S.max_pivots);
    if (lp == LP_OPTIMAL) lp = s_cut_loop(w, sh, S, e, s, rcut, min(S_RESTART_ROUNDS, S.cut_rounds), S_RESTART_PATIENCE, false);
    if (lp == LP_CUTOFF) { t.lbg = fmax(t.lbg, s.best - s_gtol(S, s.best)); s.status = MLD_STATUS_OPTIMAL; return true; }
    if (lp == LP_OPTIMAL) { s_purge_slack_cuts(w, sh); const double ob = s_objective(w, sh); if (ob > t.lbg) t.lbg = ob; }
    return false;
}

// RINS: fix the binaries on which incumbent and root relaxation agree for one pass (their root bounds saved in fx_*), and release them after it
__device__ __forceinline__ void s_rins_fix(const Ws &w, Shared &sh, const Entry &e, Tree &t)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        int nf = 0;
        for (int k = 0; k < w.nb; ++k) {
            const int j = w.bins[k];
            if (w.root_lo[j] != w.root_hi[j] && fabs(w.xroot[k] - e.v_out[j]) <= S_INTTOL) {
                w.fx_j[nf] = j; w.fx_lo[nf] = w.root_lo[j]; w.fx_hi[nf] = w.root_hi[j]; w.key[nf] = e.v_out[j]; nf++;
                w.root_lo[j] = w.root_hi[j] = e.v_out[j];
            }
        }
        sh.s_i[0] = nf;
    }
    __syncthreads();
    t.nfix = sh.s_i[0];
    MLD_CHECK(w, t.nfix >= 0 && t.nfix <= w.nb, 133, t.nfix, w.nb);
    s_set_bounds_list(w, sh, w.fx_j, w.key, w.key, t.nfix);
}

__device__ __forceinline__ void s_rins_release(const Ws &w, Shared &sh, Tree &t)
{
    __syncthreads(); if (threadIdx.x == 0) for (int k = 0; k < t.nfix; ++k) { const int j = w.fx_j[k]; w.root_lo[j] = w.fx_lo[k]; w.root_hi[j] = w.fx_hi[k]; } __syncthreads();
    s_set_bounds_list(w, sh, w.fx_j, w.fx_lo, w.fx_hi, t.nfix);
    t.rins_rounds++;
}

// Reduced-cost fixing at the true root (no temporary fixings active): a non-basic binary whose reduced cost exceeds the room below the cutoff cannot
// leave its bound in any solution that still matters; the fixing is permanent (ordered compaction -> deterministic list)
__device__ __forceinline__ void s_reduced_cost_fixing(const Ws &w, Shared &sh, double room)
{
    const int tid = threadIdx.x, n = w.n;
    const double *dd = w.dcost;
    int nfx = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += SOL_NT) {
        const int c = c0 + tid;
        bool fx = false; int j = -1; double v = 0.0;
        if (c < n) {
            j = w.nonbasic[c];
            if (j < n && w.is_int[j] && w.lo[j] != w.hi[j]) {
                const double rc = w.at_upper[c] ? -dd[c] : dd[c];
                if (rc > room + 1e-9) { fx = true; v = w.xN[c]; }
            }
        }
        int rank;
        const int tot = block_rank(sh, fx, &rank);
        if (fx) { w.sv_j[nfx + rank] = j; w.key[nfx + rank] = v; w.root_lo[j] = v; w.root_hi[j] = v; }
        nfx += tot;
    }
    __syncthreads();
    MLD_CHECK(w, nfx <= w.nb, 132, nfx, w.nb);
    if (nfx > 0) s_set_bounds_list(w, sh, w.sv_j, w.key, w.key, nfx);
}

// A node that is not pruned: its point (tmpx) and branching variable, or -- when there is none -- the evaluation of its rounded point as a leaf
__device__ __forceinline__ void s_branch_or_leaf(const Ws &w, Shared &sh, const SolverShape &S, const Entry &e, Search &s, Tree &t, Node &nd,
                                                 double obj, double cut, double inc_cut, bool qp_lp)
{
    const int tid = threadIdx.x, n = S.n, nb = S.nb;
    if (w.P && !qp_lp) { __syncthreads(); for (int j = tid; j < n; j += SOL_NT) w.tmpx[j] = w.vcur[j]; __syncthreads(); }
    else s_gather_x(w, sh, w.tmpx);
    if (!t.xroot_set) { for (int k = tid; k < nb; k += SOL_NT) w.xroot[k] = w.tmpx[w.bins[k]]; t.xroot_set = true; }
    if (t.depth == 0 && (s.have || e.ext_cut) && (t.phase == PH_IDS || t.phase == PH_FINAL) && !w.P) s_reduced_cost_fixing(w, sh, inc_cut - obj);
    if (t.phase == PH_DIVE) {   // fractional binary closest to 1 (smallest index on ties)
        double mv = -S_INF; int mi = -1;
        for (int k = tid; k < nb; k += SOL_NT) {
            const int j = w.bins[k];
            const double x = w.tmpx[j];
            // a FIXED binary is never a candidate (round 4): a basic variable with lo == hi can drift off its value by more than the integrality
            // tolerance while the primal simplex of a QP relaxation (or of s_unperturb) ignores its tiny column entries -- picked again and again
            // it made a dive of 700 levels on a 200-binary instance (oracle under ASan: the search stack overflowed; here: garbage in the
            // arrays behind stk_j, an instance ending "infeasible" with 801 nodes)
            if (fabs(x - rint(x)) > S_INTTOL && x > mv && w.lo[j] != w.hi[j]) { mv = x; mi = j; }
        }
        double tmp;
        nd.branch_j = block_argmax(sh, mv, mi, &tmp);
    } else if (!w.P && !(S.debug & MLD_DBG_FIRST_FRACTIONAL)) {
        s_penalty_branch(w, sh, w.tmpx, obj, cut, inc_cut);
        nd.branch_j = sh.s_i[0]; nd.force_first = sh.s_i[1]; nd.second_done = sh.s_i[2] != 0; nd.pen_pruned = sh.s_i[3] != 0;
        const double tn = sh.s_d[1];
        if (tn < t.t_next) t.t_next = tn;
        __syncthreads();
    } else {
        // first fractional binary in index order
        int key = 0x7fffffff;
        for (int k = tid; k < nb; k += SOL_NT) {
            const int j = w.bins[k];
            if (fabs(w.tmpx[j] - rint(w.tmpx[j])) > S_INTTOL && j < key && w.lo[j] != w.hi[j]) key = j;
        }
        nd.branch_j = block_argmin_int(sh, key, key);
    }
    MLD_CHECK(w, nd.branch_j < n, 131, nd.branch_j, t.phase);
    if (nd.branch_j >= 0) nd.branch_x = w.tmpx[nd.branch_j];
    else if (!nd.pen_pruned) {
        // leaf: fix every binary at its rounded value, re-solve, verify, restore
        MLD_MARK(w, sh, 400 + t.phase);
        const bool leaf_ok = s_leaf(w, sh, S, e, s, s.nodes);
        if (!leaf_ok) {
            // The rounded point is not feasible although every binary is within the integrality tolerance (a binary at 1e-6 can carry a whole unit
            // of a big-M row): the node is NOT a leaf -- branch on the least integral free binary (smallest index on ties).
            double mv = 1e-12; int mi = -1;
            for (int k = tid; k < nb; k += SOL_NT) {
                const int j = w.bins[k];
                const double f = fabs(w.tmpx[j] - rint(w.tmpx[j]));
                if (w.lo[j] != w.hi[j] && f > mv) { mv = f; mi = j; }
            }
            double tmp;
            nd.branch_j = block_argmax(sh, mi >= 0 ? mv : -S_INF, mi, &tmp);
            if (nd.branch_j >= 0) nd.branch_x = w.tmpx[nd.branch_j];
        }
    }
}

// One step of the dive, which does not backtrack: it ends at its first leaf, or when the node is infeasible.  Look-ahead LPs choose the child (not nodes
// of the tree: NodeLimit counts the nodes a search evaluates, as the reference's backend does -- round 4).  True: the chosen child is evaluated next.
__device__ __forceinline__ bool s_dive_step(const Ws &w, Shared &sh, const SolverShape &S, Tree &t, const Node &nd)
{
    if (nd.branch_j < 0) { t.dive_end = true; return false; }
    const int j = nd.branch_j;
    s_set_bounds(w, sh, j, 1.0, 1.0);
    const int la = s_dual_simplex(w, sh, S_INF, S.max_pivots);
    const double oa = la == LP_OPTIMAL ? s_objective(w, sh) : S_INF;
    double take = 1.0;
    if (la == LP_ITERLIMIT) t.limit = true;
    else if (!(oa <= nd.obj + t.dive_tol)) {
        s_set_bounds(w, sh, j, 0.0, 0.0);
        const int lb2 = s_dual_simplex(w, sh, S_INF, S.max_pivots);
        const double ob2 = lb2 == LP_OPTIMAL ? s_objective(w, sh) : S_INF;
        if (lb2 == LP_ITERLIMIT) t.limit = true;
        else if (ob2 <= oa) { take = 0.0; if (ob2 == S_INF) t.dive_end = true; }
        else s_set_bounds(w, sh, j, 1.0, 1.0);
    }
    __syncthreads();
    MLD_CHECK(w, t.depth >= 0 && t.depth < S.nb, 130, t.depth, 1);
    if (t.depth >= S.nb) t.limit = true;      // (cannot happen: every level holds a different free binary; the stack has nb + 2 entries)
    else { if (threadIdx.x == 0) { w.stk_j[t.depth] = j; w.stk_first[t.depth] = (unsigned char)take; w.stk_second[t.depth] = 1; } t.depth++; }
    return !t.limit && !t.dive_end;
}

// End of a pass: what a complete search leaves open is recorded or published (hand-off), then the stack is unwound (entries are distinct variables)
__device__ __forceinline__ void s_unwind(const Ws &w, Shared &sh, const SolverShape &S, const ProblemDev &P, const BatchDev &B, const Entry &e, Search &s, Tree &t, const Node &nd)
{
    const int tid = threadIdx.x, nb = S.nb, inst = e.inst;
    __syncthreads();
    const bool complete = t.complete();
    if (B.open_depth) {      // sub-tree hand-off (mld_download_open_nodes)
        if (complete)
            for (int k = tid; k < t.depth; k += SOL_NT) {
                const int j = w.stk_j[k];
                B.open_var[(size_t)inst * nb + k] = (short)j; B.open_val[(size_t)inst * nb + k] = (unsigned char)(w.lo[j] > 0.5 ? 1 : 0); B.open_flag[(size_t)inst * nb + k] = w.stk_second[k];
            }
        if (tid == 0) B.open_depth[inst] = complete ? t.depth : -1;
        __syncthreads();
    }
    if (B.ho && complete) {
        // In-kernel hand-off: this COMPLETE search stopped at its node limit.  Everything it leaves open is published as entries of the work queue;
        // whichever workgroup runs out of instances solves them (root LP and cut loop of their own, this search's incumbent as cutoff).
        t.stopped_complete = true;
        // CLOSING SWEEP before anything is published: most open siblings of a stopped search are trivial -- the warm dictionary closes
        // them in a few pivots each, an item would pay a root LP and cut rounds for the same verdict (83 % of the items of a shard at the
        // 1e-6 contract ended "nothing better in this node").  The stack is popped level by level; a level whose sibling has not been
        // visited gets that sibling's LP under the incumbent's cutoff: closed -> accounted for, still open -> it becomes an item.
        for (int k = tid; k < t.depth; k += SOL_NT) w.stk_val[k] = (unsigned char)(w.lo[w.stk_j[k]] > 0.5 ? 1 : 0);
        __syncthreads();
        const bool cur_open = nd.branch_j >= 0 || t.lp == LP_ITERLIMIT || nd.qp_open;      // (a node whose LP -- or QP relaxation -- hit the pivot limit is unsolved: still open)
        const double sweep_cut = (s.have || e.ext_cut) ? s.best - s_gtol(S, s.best) : S_INF;
        const int depth_pub = t.depth;
        if (!(S.debug & MLD_DBG_NO_SWEEP))
        for (int k = t.depth - 1; k >= 0; --k) {
            const int j = w.stk_j[k];
            if (!w.stk_second[k]) {
                const double v = 1.0 - (double)w.stk_val[k];
                s_set_bounds(w, sh, j, v, v);
                const int l2 = s_dual_simplex(w, sh, sweep_cut + 1e-12, S.max_pivots);
                s.nodes++;
                bool closed = l2 == LP_CUTOFF || l2 == LP_INFEASIBLE;
                if (l2 == LP_OPTIMAL) closed = s_objective(w, sh) > sweep_cut;
                if (l2 == LP_OPTIMAL && !closed && w.P && sweep_cut < S_INF) closed = s_sweep_close_qp(w, sh, sweep_cut, S.max_pivots);
                __syncthreads(); if (closed && tid == 0) w.stk_second[k] = 1; __syncthreads();
            }
            s_set_bounds(w, sh, j, w.root_lo[j], w.root_hi[j]);
            t.depth = k;
        }
        const int pub = s_publish_nodes(w, sh, P, B, nb, inst, e.isrc, e.is_item, e.fixed, depth_pub, true, 0, (s.have || e.ext_cut) ? s.best + e.r_const : S_INF, w.stk_val, cur_open);
        if (pub >= 0) t.expanded = t.published_rest = true;      // (0: the sweep closed everything that was open -- the search is complete)
    }
    for (int k = tid; k < t.depth; k += SOL_NT) { const int j = w.stk_j[k]; w.sv_lo[k] = w.root_lo[j]; w.sv_hi[k] = w.root_hi[j]; }
    __syncthreads();
    s_set_bounds_list(w, sh, w.stk_j, w.sv_lo, w.sv_hi, t.depth);
    t.depth = 0;
}

// The rescue: one un-thresholded dive (no clock inside its LPs) returns a feasible point; false when there is an incumbent, a cutoff, or it has run
__device__ __forceinline__ bool s_rescue(const Ws &w, Shared &sh, const Entry &e, const Search &s, Tree &t, bool refactor)
{
    if (s.have || t.rescue || e.ext_cut) return false;
    if (refactor) s_refactor(w, sh);
    if (threadIdx.x == 0) sh.deadline = 0;
    t.rescue = true; t.limit = t.timed_out = false; t.T = S_INF; t.phase = PH_FINAL; t.node_budget = s.nodes + 3 * w.nb + 10;
    return true;
}

// After a pass: the verdict, or the next pass and its phase.  Returns true when the search goes on.
__device__ __forceinline__ bool s_next_phase(const Ws &w, Shared &sh, const SolverShape &S, const Entry &e, Search &s, Tree &t)
{
    const int nb = S.nb, MAXN = e.max_nodes;
    if (t.finished) { if (s.unbounded) { s.status = MLD_STATUS_UNBOUNDED; s.best = -S_INF; } else if (!t.rescue) s.status = MLD_STATUS_OPTIMAL; return false; }
    if (t.lp == LP_ITERLIMIT && !t.timed_out) return false;      // (an LP the TimeLimit interrupted is not a pivot limit: the rescue dive still owes a feasible point)
    if (t.phase == PH_IDS && t.limit && !s.have && !t.rescue && !t.timed_out && s.nodes < MAXN && e.warm && !t.started) {
        // MIP start (mld_set_warm_start / mld_warm_start_from_previous; the reference forwards warm_start=True to its backend,
        // controller_base.py:493,509-512), evaluated lazily (oracle: same rule): only an instance whose deepening passes found no
        // incumbent pays for it (one leaf); a feasible start takes the place of the dive and the search goes on with RINS around it
        t.started = true;
        __syncthreads(); for (int k = threadIdx.x; k < nb; k += SOL_NT) w.tmpx[w.bins[k]] = (double)e.warm[k]; __syncthreads();
        MLD_MARK(w, sh, 450);
        (void)s_leaf(w, sh, S, e, s, s.nodes);
        if (s.have) { t.phase = PH_RINS; t.limit = false; t.T = S_INF; t.node_budget = min(MAXN, s.nodes + MAXN / 4); return true; }
    }
    if (t.timed_out) return s_rescue(w, sh, e, s, t, false);      // out of time: no further phase
    if (t.phase == PH_IDS && t.limit && !s.have && !t.rescue && s.nodes < MAXN) {
        // the dive may finish even when it outlasts the node budget (it is what guarantees a feasible point)
        t.phase = PH_DIVE; t.limit = false; t.T = S_INF; t.node_budget = max(MAXN, s.nodes + 3 * nb + 10); return true;
    }
    if (t.phase == PH_DIVE) {
        t.limit = s.nodes >= MAXN;
        if (s.have && !t.limit) { t.phase = PH_RINS; t.node_budget = min(MAXN, s.nodes + MAXN / 4); return true; }
        if (!s.have && !t.limit) { t.phase = PH_FINAL; t.node_budget = MAXN; return true; }
    } else if (t.phase == PH_RINS) {
        t.limit = s.nodes >= MAXN;
        if (!t.limit) {
            if (s.best < t.best_at_start && t.rins_rounds < 2) { t.node_budget = min(MAXN, s.nodes + MAXN / 4); return true; }
            t.phase = PH_FINAL; t.node_budget = MAXN; return true;
        }
    }
    if (t.limit) return s_rescue(w, sh, e, s, t, false);      // node limit
    if (s.have && s.best - s_gtol(S, s.best) <= t.T) { s.status = MLD_STATUS_OPTIMAL; return false; }
    if (t.t_next == S_INF) {
        if (s_rescue(w, sh, e, s, t, true)) return true;      // every node "infeasible": re-derive the dictionary from the original rows and dive once more
        s.status = s.have ? (t.rescue ? MLD_STATUS_NODE_LIMIT : MLD_STATUS_OPTIMAL) : MLD_STATUS_INFEASIBLE;
        return false;
    }
    if (t.t_next > t.lbg) t.lbg = t.t_next;
    if (s.have) t.T = S_INF;
    else t.T = fmax(t.t_next + 1e-9 * fmax(1.0, fabs(t.t_next)), t.T + ldexp(2.5e-4, 2 * t.pass) * fmax(1.0, fabs(t.T)));
    return true;
}

// The search below the root: passes of the phase loop, each a depth-first walk of the tree from the root, then the bound and status it proved.
__device__ __forceinline__ void s_search(const Ws &w, Shared &sh, const SolverShape &S, const ProblemDev &P, const BatchDev &B, const Entry &e, Search &s)
{
    const int tid = threadIdx.x, n = S.n, nb = S.nb, MAXN = e.max_nodes;
    for (int j = tid; j < n; j += SOL_NT) { w.root_lo[j] = w.lo[j]; w.root_hi[j] = w.hi[j]; }
    __syncthreads();
    Tree t;
    // (under an external cutoff: plain depth-first search below it; with an incumbent from an eager start: RINS around it, then the final search)
    t.node_budget = MAXN; t.phase = e.ext_cut ? PH_FINAL : (s.have ? PH_RINS : PH_IDS);
    if (tid == 0) sh.deadline = S.time_ticks > 0 ? e.t_begin + S.time_ticks : 0;      // from here on the clock is also read every 128 pivots inside an LP
    if (s.have && !e.ext_cut) {      // (the first pass is RINS: it needs the root relaxation's binaries now)
        t.started = true; t.node_budget = min(MAXN, MAXN / 4);
        s_gather_x(w, sh, w.tmpx);
        for (int k = tid; k < nb; k += SOL_NT) w.xroot[k] = w.tmpx[w.bins[k]];
        __syncthreads();
        t.xroot_set = true;
    }
    t.ids_cap = MAXN / 8 > 16 ? MAXN / 8 : 16;
    t.lbg = s.root_bound;
    t.dive_tol = 1e-2 * fmax(1.0, fabs(s.root_bound));
    t.T = (e.ext_cut || s.have) ? S_INF : s.root_bound + fmax(1e-7 * fmax(1.0, fabs(s.root_bound)), s_gtol(S, s.root_bound));
    s.status = MLD_STATUS_NODE_LIMIT; s.nodes = 0;
    do {
        t.depth = 0; t.t_next = S_INF; t.finished = t.dive_end = false; t.best_at_start = s.best; t.pass++;
        MLD_MARK(w, sh, 100 + 10 * t.phase + (t.pass < 10 ? t.pass : 9));
        if (s_root_restart(w, sh, S, e, s, t)) break;
        if (t.phase == PH_RINS) s_rins_fix(w, sh, e, t);
        for (;;) {
            s.nodes++;
            Node nd;
            // RINS is a heuristic on a sub-problem: it keeps ANY improvement (round 4; oracle: same rule).  With the proof's cutoff -- "better by more than the
            // gap" -- it threw away exactly the points that matter at the cfg5 size: the dive's leaf is 0.5-1 % above the best point, the root bound within 1 % of THAT one
            const double inc_cut = (s.have || e.ext_cut) ? ((t.phase == PH_RINS && s.have) ? s.best - 1e-6 * fmax(1.0, fabs(s.best)) : s.best - s_gtol(S, s.best)) : S_INF;
            const double cut = fmin(t.T, inc_cut);
            if (S.debug & MLD_DBG_TRACE) s_debug_dual(w, sh, e.inst, "node entry");
            t.lp = s_dual_simplex(w, sh, cut + 1e-12, S.max_pivots);
            if (S.debug & MLD_DBG_TRACE) s_debug_dual(w, sh, e.inst, "node exit");
            if ((S.debug & MLD_DBG_TRACE) && tid == 0) MLD_PRINTF("[inst %d] node %d ph %d depth %d lp=%d obj=%.12g cut=%.12g T=%.12g pivots=%d\n", e.inst, s.nodes, t.phase, t.depth, t.lp, s_objective_nosync(w), cut, t.T, sh.pivots);
            if (t.lp == LP_ITERLIMIT) t.limit = true;
            else if (t.lp == LP_OPTIMAL || t.lp == LP_CUTOFF) {
                double obj = s_objective(w, sh);      // LP(q) value: a valid bound also when P is PSD
                bool pruned = (t.lp == LP_CUTOFF || obj > cut), qp_lp = false;
                nd.obj = obj;
                if (!pruned && w.P) {
                    double lbq, fvq;
                    const int rc = s_sd_relax(w, sh, cut, S.max_pivots, &lbq, &fvq);
                    if (rc == -1) { t.limit = true; pruned = true; obj = S_INF; nd.qp_open = true; }
                    else if (rc == -2) qp_lp = true;      // the QP relaxation could not be finished: this node goes on with its LP(q) bound and LP point
                    else { obj = lbq; pruned = (rc == 1 || obj > cut); }
                }
                if (pruned) { if (obj <= inc_cut && obj < t.t_next) t.t_next = obj; }
                else s_branch_or_leaf(w, sh, S, e, s, t, nd, obj, cut, inc_cut, qp_lp);
            }
            if (s.have && (t.rescue || s.unbounded || s.best <= t.lbg + s_gtol(S, s.best))) t.finished = true;
            if (s.nodes >= ((t.phase == PH_IDS && !s.have && !t.rescue) ? t.ids_cap : t.node_budget)) {
                t.limit = true;
                if (B.ho && B.ho_donate > 0 && t.donations < B.ho_rounds && t.lp != LP_ITERLIMIT && !nd.qp_open && t.complete()) {
                    // Node limit inside a complete search with the in-kernel hand-off on: give the LARGEST open subtrees away -- the shallowest
                    // open siblings of the stack become items for idle workgroups -- and go on below them with a new budget.  What stays here are
                    // the deep open nodes, which this dictionary closes in a few pivots each; an item pays a root LP and a cut loop of its own.
                    const int given = s_publish_nodes(w, sh, P, B, nb, e.inst, e.isrc, e.is_item, e.fixed, t.depth, false, B.ho_donate, (s.have || e.ext_cut) ? s.best + e.r_const : S_INF, nullptr, false);
                    if (given > 0) t.expanded = true;
                    t.donations++;
                    t.node_budget = s.nodes + B.ho_sub_nodes;
                    t.limit = false;
                }
            }
            if (S.time_ticks > 0 && !t.rescue) {      // TimeLimit (the reference forwards it per call, micro_grid_control_simulation.py:232): ends the search like the node limit
                __syncthreads(); if (tid == 0) sh.s_i[4] = (wall_clock64() - e.t_begin > S.time_ticks) ? 1 : 0; __syncthreads();
                if (sh.s_i[4]) { t.limit = true; t.timed_out = true; }
            }
            if (t.phase == PH_DIVE && !t.limit && !t.finished && s_dive_step(w, sh, S, t, nd)) continue;     // evaluate the chosen child
            if (nd.branch_j >= 0 && t.depth >= nb) t.limit = true;      // (cannot happen, see the dive: the search ends rather than write behind its stack)
            if (nd.branch_j >= 0 && !t.limit && !t.finished && !t.dive_end) {
                double first = nd.force_first >= 0 ? (double)nd.force_first : (nd.branch_x >= 0.5 ? 1.0 : 0.0);
                if (s.have && t.phase == PH_FINAL && !nd.second_done) first = rint(e.v_out[nd.branch_j] / w.cs[nd.branch_j]);   // guided (Danna et al. 2005): towards the incumbent first
                __syncthreads();
                MLD_CHECK(w, t.depth >= 0 && t.depth < nb && (first == 0.0 || first == 1.0), 130, t.depth, (int)(first * 1000));
                if (tid == 0) { w.stk_j[t.depth] = nd.branch_j; w.stk_first[t.depth] = (unsigned char)first; w.stk_second[t.depth] = nd.second_done ? 1 : 0; }
                t.depth++;
                s_set_bounds(w, sh, nd.branch_j, first, first);
                continue;
            }
            if (t.limit || t.finished || t.dive_end) { s_unwind(w, sh, S, P, B, e, s, t, nd); break; }
            __syncthreads();
            while (t.depth > 0 && w.stk_second[t.depth - 1]) { t.depth--; const int j = w.stk_j[t.depth]; s_set_bounds(w, sh, j, w.root_lo[j], w.root_hi[j]); }
            if (t.depth == 0) break;
            __syncthreads();
            if (tid == 0) w.stk_second[t.depth - 1] = 1;
            { const int j = w.stk_j[t.depth - 1]; const double v = 1.0 - (double)w.stk_first[t.depth - 1]; s_set_bounds(w, sh, j, v, v); }
        }
        if (t.phase == PH_RINS) s_rins_release(w, sh, t);
    } while (s_next_phase(w, sh, S, e, s, t));
    // every way of ending OPTIMAL has closed all nodes below best - gtol; otherwise the bound is what exhaustive passes proved
    s.lb_proven = s.status == MLD_STATUS_OPTIMAL ? fmin(s.best, fmax(t.lbg, s.best - s_gtol(S, s.best))) : t.lbg;
    if (B.ho && !t.expanded && !t.stopped_complete && s.status == MLD_STATUS_NODE_LIMIT && s.have) {
        // The search stopped at a limit BEFORE it became a plain depth-first search below an incumbent (deepening passes, dive, RINS): no stack
        // describes what is left, so its one open node is its own root -- published once more, now under the incumbent's value as cutoff (the
        // item starts as a complete search and can be split).  Without an incumbent there is nothing to gain from running the same search again.
        if (s_publish_nodes(w, sh, P, B, nb, e.inst, e.isrc, e.is_item, e.fixed, 0, true, 0, s.best + e.r_const, nullptr, true) > 0) t.expanded = t.published_rest = true;
    }
    if (t.expanded) {
        // (internal statuses, merged by k_merge_*: what this entry left open lives on as its items.  Its own rest is closed when the search ended on its
        // own, or when everything that was left went into items; the bound it reports is the one that holds for its WHOLE node -- a search that
        // gave subtrees away has proven nothing about them)
        if (s.status == MLD_STATUS_OPTIMAL || s.status == MLD_STATUS_INFEASIBLE || (s.status == MLD_STATUS_NODE_LIMIT && t.published_rest)) s.status = MLD_STATUS_EXPANDED;
        else if (s.status == MLD_STATUS_NODE_LIMIT) s.status = MLD_STATUS_EXPANDED_OPEN;
        s.lb_proven = t.lbg;
    }
}

// Write-out: the entry's results (a SKIPPED item reports no work), then, with the in-kernel hand-off, the entry is counted as finished once its results
// and any items it published are visible: the launch ends when finished == tail.
__device__ __forceinline__ void s_write_results(Shared &sh, const BatchDev &B, const Entry &e, const Search &s)
{
    const bool skipped = s.status == MLD_STATUS_SKIPPED;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int inst = e.inst;
        B.obj_out[inst] = s.have ? s.best + e.r_const : S_INF;
        B.lb_out[inst] = s.lb_proven + e.r_const;
        B.status_out[inst] = s.status;
        B.nodes_out[inst] = s.nodes; B.pivots_out[inst] = skipped ? 0 : sh.pivots; B.cuts_out[inst] = s.cuts; B.refac_out[inst] = skipped ? 0 : sh.refactors;
        B.ticks_out[inst] = skipped ? 0 : wall_clock64() - e.t_begin; B.rows_out[inst] = skipped ? 0 : (long long)sh.rows;
#ifdef MLD_PIVOT_PROF
        // (-DMLD_PIVOT_PROF: the clocks of the pivot's sub-phases; -DMLD_PIVOT_PROF=2: the counts and the long-step clock of the same launch instead -- scripts/gpu_pivot_prof.py)
        // (-DMLD_PIVOT_PROF=3 / =4: the selection's sub-clocks of the loop / of the look-ahead in slots 0 .. 4 / 0 .. 3, the selection clock itself in slot 7)
        if (B.prof_out && !skipped) for (int k = 0; k < 8; ++k)
            B.prof_out[(size_t)inst * 8 + k] = MLD_PIVOT_PROF == 2 ? sh.pcnt[k] : MLD_PIVOT_PROF == 3 ? (k < 5 ? sh.sprof[k] : k == 7 ? sh.prof[1] : 0)
                                             : MLD_PIVOT_PROF == 4 ? (k < 4 ? sh.sprof[5 + k] : k == 7 ? sh.prof[1] : 0) : sh.pprof[k];
#else
        if (B.prof_out && !skipped) for (int k = 0; k < 8; ++k) B.prof_out[(size_t)inst * 8 + k] = sh.prof[k];
#endif
#ifdef MLD_CUT_PROF
        if (B.prof_out && !skipped) { B.prof_out[(size_t)inst * 8 + 3] = sh.cprof[0]; B.prof_out[(size_t)inst * 8 + 4] = sh.cprof[1]; B.prof_out[(size_t)inst * 8 + 7] = sh.cprof[2]; }   // (diagnostic build: slots 3 / 4 / 7 = c-MIR scoring / c-MIR build / Gomory)
#if MLD_CUT_PROF == 2
        if (B.prof_out && !skipped) for (int k = 0; k < 8; ++k) B.prof_out[(size_t)inst * 8 + k] = sh.cprof[3 + k];      // (the counts instead: scripts/gpu_cut_prof.py counts)
#endif
#if MLD_CUT_PROF == 3
        if (B.prof_out && !skipped) { for (int k = 0; k < 4; ++k) B.prof_out[(size_t)inst * 8 + k] = sh.cprof[11 + k]; B.prof_out[(size_t)inst * 8 + 4] = sh.cprof[0]; B.prof_out[(size_t)inst * 8 + 5] = sh.prof[2]; }      // (phase A's sub-clocks, phase A, all cut separation: scripts/gpu_walks_prof.py)
#endif
#endif
    }
    if (B.ho) { __threadfence(); __syncthreads(); if (threadIdx.x == 0) __hip_atomic_fetch_add(B.finished, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }
}

__global__ void __launch_bounds__(SOL_NT, SOL_WPE) k_solve(SolverShape S, ProblemDev P, BatchDev B, unsigned char *ws_base)
{
    extern __shared__ double lds[];
    __shared__ Shared sh;
    __shared__ int s_inst, s_dead;
    const int tid = threadIdx.x;
    Ws w;
    s_bind_slot(w, S, ws_base + (size_t)blockIdx.x * S.ws_stride, lds);
    for (;;) {
        __syncthreads();
        if (tid == 0) {
            int q = atomicAdd(B.counter, 1);
            if (B.ho && q >= B.batch) {
                // Entry q of the queue is an item that may not have been published yet.  Wait for it, or for the end of the launch: no entry is being
                // worked on and none can appear any more once finished == tail (entries are reserved only by workgroups that work on one; tail and
                // finished only grow, so equal reads of tail around a read of finished give the value at one instant).  Every workgroup of the grid
                // reaches one of the two exits: a running entry always ends (node / pivot limits), and the last one to end makes finished == tail.
                for (;;) {
                    if (q < B.cap && __hip_atomic_load(&B.item_ready[q], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) break;
                    const int t1 = __hip_atomic_load(B.tail, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                    const int f = __hip_atomic_load(B.finished, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                    const int t2 = __hip_atomic_load(B.tail, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                    if (t1 == t2 && f == t1 && q >= t1) { q = -1; break; }
                    __builtin_amdgcn_s_sleep(64);
                }
            } else if (q >= B.batch) q = -1;
            s_inst = q;
            // (read by ONE thread and broadcast: the flag can change at any moment, and the workgroup must agree)
            s_dead = (B.ho && q >= B.batch) ? __hip_atomic_load(&B.tree_dead[B.item_root[q]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        }
        __syncthreads();
        if (s_inst < 0) break;
        if (B.ho) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");             // an item's data was written by another workgroup (every wave: its own view)
        Entry e;
        e.inst = (B.order && s_inst < B.batch) ? B.order[s_inst] : s_inst; e.is_item = B.ho && s_inst >= B.batch;
        e.isrc = e.is_item ? B.item_src[e.inst] : e.inst; e.max_nodes = e.is_item ? B.ho_sub_nodes : S.max_nodes;
        Search s;
        if (e.is_item && s_dead) {
            // the tree this item belongs to has been given up (too many open nodes): nothing of it is solved any more
            s.status = MLD_STATUS_SKIPPED; s.nodes = 0; e.r_const = 0.0;
        } else {
            w.trace = B.trace ? B.trace + (size_t)blockIdx.x * 16 : nullptr;
            if (w.trace && tid == 0) { w.trace[0] = e.inst; w.trace[1] = 1; w.trace[2] = 0; w.trace[3] = s_inst; __threadfence_system(); }
            MLD_CHECK(w, e.inst >= 0 && e.inst < B.batch, 129, e.inst, s_inst);
            MLD_CHECK(w, !(S.debug & MLD_DBG_ASSERT_POSCTL), 999, e.inst, s_inst);      // (positive control of the assertion build: this one fails)
            if (s_setup_entry(w, sh, S, P, B, e, s) && s_root(w, sh, S, e, s)) s_search(w, sh, S, P, B, e, s);
            MLD_MARK(w, sh, 999);
        }
        s_write_results(sh, B, e, s);
    }
}

// Diagnostics (mld_debug_reduce): the block reductions of the selection on caller-supplied vectors of SOL_NT (value, index) lanes, a workgroup per vector -- the
// primitives over __shfl_down (slot 0) and the DPP ones that replaced them in the simplex loop (slot 1): max2[2 b + s] the block maximum, arg2 / val2 the arg-max
// and its value.  Three reductions each, alternating buffers as in the loop.
__global__ void __launch_bounds__(SOL_NT) k_debug_reduce(const double *v, const int *idx, double *max2, int *arg2, double *val2)
{
    __shared__ Shared sh;
    const size_t b = blockIdx.x;
    const double x = v[b * SOL_NT + threadIdx.x];
    const int i = idx[b * SOL_NT + threadIdx.x];
    int par = 0;
    double o0, o1;
    const double m0 = block_max1(sh, x, par), m1 = block_max1_dpp(sh, x, par);
    const int a0 = block_argmax1(sh, x, i, &o0, par), a1 = block_argmax1_dpp(sh, x, i, &o1, par);
    const double n0 = block_min1(sh, x, par), n1 = block_min1_dpp(sh, x, par);
    if (threadIdx.x == (blockIdx.x & (SOL_NT - 1))) {      // (every thread holds the results: another thread reports for every vector)
        max2[2 * b] = m0; max2[2 * b + 1] = m1; arg2[2 * b] = a0; arg2[2 * b + 1] = a1; val2[2 * b] = o0; val2[2 * b + 1] = o1;
        max2[2 * gridDim.x + 2 * b] = n0; max2[2 * gridDim.x + 2 * b + 1] = n1;
    }
}

// Diagnostics (mld_debug_update_rows): the rows' update of ONE pivot (pair == 0) or of a fused pair on a caller-supplied dictionary D (m x ld) with the staged
// rows and multiplier columns the caller gives -- the lists are built and the update runs through s_pivot_update / s_pair_update themselves: the templates the
// default loop runs or, with MLD_DBG_UPDATE_R7 (and MLD_DBG_PIVOT_SYNC_R5) in dbg, the earlier ones.  One workgroup; rows_out = the (row, sector) pairs accounted.
#define DBG_UPD_MAX 1024      // rows and leading dimension the static LDS of this kernel holds
__global__ void __launch_bounds__(SOL_NT) k_debug_update(double *D, int m, int n, int ld, const double *rowr1, const double *colc1, int r1, int c1,
                                                         const double *rowr2, const double *colc2, int r2, int c2, int pair, int dbg, unsigned long long *rows_out)
{
    __shared__ Shared sh;
    __shared__ double s_rowr[2][DBG_UPD_MAX + 8], s_colc[2][DBG_UPD_MAX + 8];
    __shared__ unsigned short s_sec[2][DBG_UPD_MAX / SOL_SEC + 8], s_row[2][DBG_UPD_MAX + 8];
    __shared__ unsigned char s_flag[DBG_UPD_MAX / SOL_SEC + 8];
    const int tid = threadIdx.x;
    Ws w = {};
    w.D = D; w.n = n; w.ld = ld; w.mcap = m; w.m0 = m; w.dbg = dbg;
    w.rowr = s_rowr[0]; w.colc = s_colc[0]; w.seclist = s_sec[0]; w.rowlist = s_row[0];
    w.rowr2 = s_rowr[1]; w.colc2 = s_colc[1]; w.seclist2 = s_sec[1]; w.rowlist2 = s_row[1]; w.secflag = s_flag; w.pair = pair;
    if (tid == 0) { sh.m = m; sh.rows = 0ull; sh.prof[0] = 0; }
    for (int k = tid; k < ld; k += SOL_NT) { s_rowr[0][k] = k <= n ? rowr1[k] : 0.0; s_rowr[1][k] = (pair && k <= n) ? rowr2[k] : 0.0; }      // (the last sector's padding: 0)
    for (int i = tid; i < m; i += SOL_NT) { s_colc[0][i] = colc1[i]; if (pair) s_colc[1][i] = colc2[i]; }
    __syncthreads();
    const long long tp0 = wall_clock64();
    if (pair) {
        for (int t = tid; t < (n + SOL_SEC) / SOL_SEC; t += SOL_NT) {      // active sectors of the first pivot's row (as s_pivot_pair marks them)
            bool act = false;
#pragma unroll
            for (int e = 0; e < SOL_SEC; ++e) { const int k = t * SOL_SEC + e; if (k <= n && s_rowr[0][k] != 0.0) act = true; }
            s_flag[t] = act ? 1 : 0;
        }
        __syncthreads();
        s_pair_update<true>(w, sh, r1, c1, r2, c2, tp0);      // (the instantiation that chooses by w.dbg: without a bit it runs what the default loop runs)
    } else {
        s_pivot_update<true>(w, sh, r1, c1, tp0);
    }
    __syncthreads();
    if (tid == 0) *rows_out = sh.rows;
}
