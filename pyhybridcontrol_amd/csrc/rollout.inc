// k_rollout: open-loop rollout of plans under realised disturbances (mld_rollout_batch) -- the reference's MldModel.lsim, or lsim_k in a loop
// (models/mld_model.py:543-642, 647-699), with _compute_aux (:701-766) re-deriving delta, z, mu at every step: what the hybrid plant does over the next K
// steps when the inputs u_0 .. u_{K-1} are applied and the disturbance turns out to be realisation c.  A trajectory is (instance b, realisation c),
// t = b S + c; per step k
//     omega' = [omega_k; u_k],  h_i = rs_i (Hx[i,:] x + Hw[i,:] omega' + H5[i])          the resolver's right-hand side (K3 up to summation order)
//     sm_solve on the resolver's scaled, tightened rows with h: min sum(mu)                (small_lds.inc, unchanged)
//     v_k = [u_k; delta; z; mu],  x_{k+1}, y_k, r by the functions k_sim_step calls        (plant_step.inc: the one definition of the sums)
// and x never leaves the wave.  The state, omega', h, v_k, y and the next state are staged in the wave's LDS behind the solver's region:
//     [x (nx) | omega' (nomega + nu) | h (m) | v_k (nv) | y (ny) | x_{k+1} (nx)]
// (the last block because a lane's rows of x_{k+1} are ready while other lanes still read x).
//
// Mapping: one 64-lane wave per trajectory, SM_WAVES per workgroup, trajectories claimed from an atomic counter exactly as k_small_milp claims instances
// (sm_claim: every lane takes part, no lane-dependent branch between the write-out and the broadcast); the waves share nothing and the kernel holds
// no __syncthreads.  All arithmetic is fp64 on the ORIGINAL matrices of mld_model::d_pack and the resolver's fp64 maps, also on an MLD_F32 handle.  No
// dimension is a compile-time constant: rows and columns are looped lane, lane + 64, ...  Every store is lane-contiguous.
//
// The per-trajectory core ro_run compiles for the host as sm_solve does (SM_HOST: a "wave" is one lane, the staging plain memory).
//
// k_rollout_policy (mld_rollout_policy) is the second instantiation of the same body: ro_run<true> replaces step 1's copy of u_k by a feedback rule
// u_k = f(x_k, u_{k-1}) per input channel -- the reference's thermostat, DewhTheromstatController.feedback (examples/residential_mg_with_pv_and_dewhs/
// controllers/theromstat_control.py:38-64), stepped through sim_step_k --, lanes on channels, the selector row summed over x in LDS, u_{k-1} read from v's
// own block before the lane overwrites it: the staging grows by nothing.  The tables are read from global memory per step, nu (nx + 5) doubles per model:
// per channel [sel (nx) | on_at | off_at | u_on | u_off | mode].  The flag is a template parameter; the open-loop instantiation compiles to what it compiled to.
//
// k_rollout_kpi / k_rollout_policy_kpi (mld_rollout_kpi) are the same body with ro_run's second flag: the campaign's column statistics (log_summary.inc: THE
// RULE) of every trajectory, reduced where its records already lie.  In step 5 the record of step k -- x_k, v_k, y_k, omega_k, x_{k+1} -- is the staging itself
// (xs, vs, ys, ws[0 .. nw), xn), so lane q < n_kpi evaluates KPI q from LDS (every lane the same address: broadcasts) against the weights k_log_summary reads,
// (n_models, rows, n_kpi) KPI-minor, by the functions k_log_summary calls: the figures are the ones the logged stepwise route gives, bit for bit, and the only
// new HBM traffic is the weights (cached) and one price per step.  A priced KPI multiplies by lib[price_start[b] + (step + k) n_chan + ch], the price
// sim_step(step = step + k) records.  The accumulators live in the wave's LDS behind x_{k+1}, 6 n_kpi doubles [sum | min | max | prev | min_step, max_step |
// n_above, n_changes] (ro_stage_doubles): across sm_solve they cost no register -- k_rollout already spills at its bound -- and with SM_HOST one lane walks all
// n_kpi of them.  A trajectory that does not end 0 gets NaN / -1.
//
// DEVICE COMPLETION of declined trajectories (mld_set_rollout_completion; k_ro_collect, k_rollout_redo[_kpi], k_ro_fix_merge) -- THE RULE, that of
// mld_sim_step_resolve applied inside a trajectory.  A trajectory t that ended 2 is re-run FROM STEP 0 by the same ro_run body (its third flag, FIX), every sum
// in its order.  Entry e of the call's list of declined trajectories owns a table of K answers (delta, z, mu: n doubles each) and K marks.  At a step whose mark
// is RO_FIX_ANSWER ro_run takes delta, z, mu from the table instead of calling sm_solve; at one marked RO_FIX_NO_POINT it ends 1 there, NaN / -1 from there on.
// At the first step k where sm_solve declines and the table has no answer the wave writes the resolver inputs of that step -- x_k and [omega_k; u_k], under a
// policy the rule's u_k: the bytes k_aux_inputs writes for mld_sim_step_resolve(u0 = u_k) at that state -- into its slot of the resolver's input buffers,
// records k and ends 2 again.  The host then solves the listed slots on the resolver's handle with the DENSE kernel, the small path bypassed (a slot's bits do
// not depend on its neighbours), and k_ro_fix_merge makes the answer entry (e, k): usable -- status 0 or 2 with a finite objective and finite values, the rule
// of BatchAuxResolver.resolve and simlog.rollout_continue -- or "no feasible point".  Rounds repeat while a trajectory is still 2; each moves every listed
// trajectory's declining step strictly forward, so there are at most K of them and one more re-run (the loop is bounded by K in code).  The steps before k
// are re-solved by the same deterministic LDS solver to the same bits: no resume record, nothing on the common path, nothing added to the eight kernels above.
// The re-run kernel is the superset body -- candidates, a policy table per candidate, FIX -- in two instantiations, without and with the KPIs: an open-loop
// trajectory reads the table whose every channel is passed through, which reproduces ro_run<false> bit for bit.
#pragma once

#include "plant_step.inc"
#include "small_lds.inc"
#include "log_summary.inc"

struct RoModel {      // one trajectory's model: the step matrices inside the packed block, the resolver's maps and row scales
    int nx, nu, nw, nv, nmu, ny, nc;
    int m, n;                                                              // the resolver's rows and unknowns (n = ndelta + nz + nmu; 0: nothing to resolve)
    PlantMats P;                                                           // the step matrices inside the model's packed block (plant_mats)
    const double *Hx, *Hw, *H5, *rs;                                       // m x nx, m x (nw + nu), m, m
    const double *pol;                                                     // ro_run<true>: the model's policy table, nu x (nx + 5)
};
struct RoTraj {       // one trajectory's inputs and outputs (any output may be null)
    int K;
    const double *x0;                                                      // nx
    const double *u; size_t u_step;                                        // u_k = u + k u_step
    const double *om;                                                      // K x nw
    const double *cw;                                                      // K x nv or null
    double *x, *v, *y, *vio; int *row;                                     // (K + 1) x nx, K x nv, K x ny, K, K
    const double *u_prev;                                                  // ro_run<true>: nu, the input before step 0
};
struct RoResult { double cost, mu_total, worst_vio; int worst_step, worst_row, steps_done, end_status, switches; };
struct RoKpi {        // ro_run<., true>: one trajectory's KPIs (log_summary.inc: THE RULE)
    int n_kpi, n_chan;
    unsigned given;                                                        // bit t: table t of x, v, y, omega, x_k1 is given
    const double *W, *thresh;                                              // the model's (rows, n_kpi) KPI-minor, rows = the widths of the given tables, and (n_kpi)
    const int *price_chan;                                                 // n_kpi, -1 = not priced
    const double *price;                                                   // the instance's price of step 0, channel 0: step k, channel c at price[k n_chan + c]; null = none priced
    double vio_tol;
    double *sum, *min, *max; int *min_step, *max_step, *n_above, *n_changes, *n_vio;      // the trajectory's n_kpi entries each, n_vio one
};
struct RoFix {        // ro_run<., ., true>: one listed trajectory's table and its slot of the resolver's inputs (DEVICE COMPLETION above)
    const double *ans;                                                     // K x n: delta, z, mu of the steps the dense solver has answered
    const int *mark;                                                       // K: RO_FIX_OPEN, RO_FIX_ANSWER or RO_FIX_NO_POINT
    double *ax0, *aom;                                                     // the slot's rows of the resolver's inputs: nx, nw + nu
    int *step;                                                             // out: the step whose inputs were written, -1 for a trajectory that ended 0 or 1
};
enum { RO_FIX_OPEN = 0, RO_FIX_ANSWER = 1, RO_FIX_NO_POINT = 2 };
enum { RO_COMPLETE = 0, RO_INFEASIBLE = 1, RO_DECLINED = 2, RO_NOT_ATTEMPTED = -1 };
enum { POL_ON_AT = 0, POL_OFF_AT = 1, POL_U_ON = 2, POL_U_OFF = 3, POL_MODE = 4, POL_TAIL = 5 };      // a channel's table row behind its nx selector entries

// The rule of one ruled channel (theromstat_control.py:53-58, in that order): tab = the channel's row, s = sel . x with i ascending.  A NaN s falls through
// to the comparison with the previous input, as it does in the reference; with on_at == off_at the first line wins.
template <typename X> SM_FN double policy_rule(const double *tab, int nx, const X *x, double prev)
{
    double s = 0.0;
    for (int i = 0; i < nx; ++i) s += tab[i] * x[i];
    const double *t = tab + nx;
    if (s <= t[POL_ON_AT]) return t[POL_U_ON];
    if (s >= t[POL_OFF_AT]) return t[POL_U_OFF];
    return prev == t[POL_U_ON] ? t[POL_U_ON] : t[POL_U_OFF];
}

// The table a candidate of mld_rollout_select_policy reads, among the P - n_seq + 1 tables of the call: policy candidate cp >= n_seq its own, cp - n_seq; a
// plan or sequence candidate the last one, whose every channel is passed through (mode 0) -- ro_run<true> with it copies u_k as ro_run<false> does and
// counts no switch.  One index computation: no branch around ro_run.
SM_FN size_t ro_cand_table(int cp, int n_seq, int P) { return (size_t)(cp >= n_seq ? cp - n_seq : P - n_seq); }
// the rows of candidate cp for an instance of model mdl inside the tables (P - n_seq + 1, n_models, tab_len)
SM_FN const double *ro_cand_rows(const double *tabs, size_t tab_len, int n_models, int cp, int n_seq, int P, int mdl)
{
    return tabs + (ro_cand_table(cp, n_seq, P) * (size_t)n_models + (size_t)mdl) * tab_len;
}
// Step 0 of policy candidate `pick` on channel j (k_select_inputs): policy_rule on the instance's x0 and u_prev[j], the call step 0 of ro_run<true> makes
template <typename X> SM_FN double ro_cand_input(const double *tabs, size_t tab_len, int n_models, int pick, int n_seq, int P, int mdl, int j, int nx, const X *x0, double u_prev_j)
{
    return policy_rule(ro_cand_rows(tabs, tab_len, n_models, pick, n_seq, P, mdl) + (size_t)j * (size_t)(nx + POL_TAIL), nx, x0, u_prev_j);
}

// doubles of staging behind the solver's region (even, so that the next wave's region stays 16-byte aligned)
static inline size_t ro_stage_doubles(int nx, int nu, int nw, int m, int nv, int ny, int n_kpi = 0)
{
    return ((size_t)2 * nx + nw + nu + m + nv + ny + (size_t)6 * n_kpi + 1) & ~(size_t)1;
}

// The KPI accumulators of a trajectory in its staging, KPI q at [q] of each run (lane-contiguous, no bank shared): four runs of doubles, then two of int pairs
struct RoKpiAcc { sm_f64 *sum, *min, *max, *prev; sm_i32 *steps, *counts; };
SM_FN RoKpiAcc ro_kpi_acc(sm_f64 *as, int Q)
{
    RoKpiAcc a;
    a.sum = as; a.min = as + Q; a.max = as + 2 * Q; a.prev = as + 3 * Q; a.steps = (sm_i32 *)(as + 4 * Q); a.counts = (sm_i32 *)(as + 5 * Q);
    return a;
}

// the trajectory's KPI outputs: its accumulators, or NaN / -1 for one that did not end 0 (as == nullptr); lane q writes entry q
SM_FN void ro_kpi_write(const RoKpi &Q, sm_f64 *as, int lane, int n_vio)
{
    const double qnan = __builtin_nan("");
    if (as) {
        const RoKpiAcc a = ro_kpi_acc(as, Q.n_kpi);
        for (int q = lane; q < Q.n_kpi; q += SM_W) {
            Q.sum[q] = a.sum[q]; Q.min[q] = a.min[q]; Q.max[q] = a.max[q];
            Q.min_step[q] = a.steps[2 * q]; Q.max_step[q] = a.steps[2 * q + 1]; Q.n_above[q] = a.counts[2 * q]; Q.n_changes[q] = a.counts[2 * q + 1];
        }
    } else
        for (int q = lane; q < Q.n_kpi; q += SM_W) {
            Q.sum[q] = Q.min[q] = Q.max[q] = qnan;
            Q.min_step[q] = Q.max_step[q] = Q.n_above[q] = Q.n_changes[q] = -1;
        }
    if (lane == 0) *Q.n_vio = as ? n_vio : -1;
}

// everything after step `from` of a trajectory that stopped there: NaN / -1
SM_FN void ro_blank(const RoModel &M, const RoTraj &T, int lane, int from, bool with_state)
{
    const double qnan = __builtin_nan("");
    const size_t left = (size_t)(T.K - from);
    if (T.x) { const size_t o = (size_t)(with_state ? from : from + 1) * M.nx; for (size_t e = lane; e < (size_t)(T.K + 1) * M.nx - o; e += SM_W) T.x[o + e] = qnan; }
    if (T.v) for (size_t e = lane; e < left * M.nv; e += SM_W) T.v[(size_t)from * M.nv + e] = qnan;
    if (T.y) for (size_t e = lane; e < left * M.ny; e += SM_W) T.y[(size_t)from * M.ny + e] = qnan;
    if (T.vio) for (size_t e = lane; e < left; e += SM_W) T.vio[from + e] = qnan;
    if (T.row) for (size_t e = lane; e < left; e += SM_W) T.row[from + e] = -1;
}

// One trajectory, start to finish.  mem: the solver's region (S.wave_doubles doubles), stg: the staging (ro_stage_doubles); A: the resolver's model
// (G, q, lb, ub, cs, is_int, bins), its h / v_out / fixed are set here.  POLICY: the ruled channels of u_k come from M.pol, x_k and u_{k-1} (T.u_prev before
// step 0); T.u supplies the passed-through channels only, and R.switches counts the (step, ruled channel) pairs whose input changed.  KPI: Q's statistics of
// the trajectory's records are accumulated in the staging behind x_{k+1} and written by the end (every output of Q is written; stg holds ro_stage_doubles
// with Q->n_kpi).  FIX: step 3 reads F's table where it has an entry and solves where it has none; a decline there writes the step's resolver inputs (THE RULE
// of the device completion, in the header).
template <bool POLICY = false, bool KPI = false, bool FIX = false>
SM_FN void ro_run(const SmShape &S, const RoModel &M, sm_f64 *mem, sm_f64 *stg, SmArgs A, const RoTraj &T, int lane, RoResult &R, const RoKpi *Q = nullptr,
                  [[maybe_unused]] const RoFix *F = nullptr)
{
    const int nx = M.nx, nu = M.nu, nw = M.nw, nv = M.nv, ny = M.ny, nc = M.nc, m = M.m, nw2 = M.nw + M.nu, nf = M.nv - M.nmu;
    sm_f64 *xs = stg, *ws = xs + nx, *hs = ws + nw2, *vs = hs + m, *ys = vs + nv, *xn = ys + ny;
    const PlantMats &P = M.P;
    const double qnan = __builtin_nan("");
    A.h = (const double *)hs; A.v_out = (double *)(vs + nu); A.fixed = nullptr;
    for (int j = lane; j < nx; j += SM_W) { const double t = T.x0[j]; xs[j] = t; if (T.x) T.x[j] = t; }
    if constexpr (POLICY) for (int j = lane; j < nu; j += SM_W) vs[j] = T.u_prev[j];      /* u_{-1}: a lane reads and writes its own channels only */
    double cost = 0.0, mu_total = 0.0, worst = -S_INF;
    int wstep = -1, wrow = -1, end = RO_COMPLETE, k = 0;
    [[maybe_unused]] int sw = 0, n_vio = 0;
    if constexpr (KPI) {      /* a lane initialises the accumulators it alone reads and writes */
        const RoKpiAcc a = ro_kpi_acc(xn + nx, Q->n_kpi);
        for (int q = lane; q < Q->n_kpi; q += SM_W) {
            LsAcc c; ls_acc_init(c);
            a.sum[q] = c.sum; a.min[q] = c.min; a.max[q] = c.max; a.prev[q] = c.prev;
            a.steps[2 * q] = c.min_step; a.steps[2 * q + 1] = c.max_step; a.counts[2 * q] = c.n_above; a.counts[2 * q + 1] = c.n_changes;
        }
    }
    for (; k < T.K; ++k) {
        // ---- 1. the step's inputs
        const double *uk = T.u + (size_t)k * T.u_step, *wk = T.om + (size_t)k * nw;
        sm_sync();
        for (int j = lane; j < nw; j += SM_W) ws[j] = wk[j];
        if constexpr (POLICY) {
            for (int j = lane; j < nu; j += SM_W) {
                const double *tab = M.pol + (size_t)j * (nx + POL_TAIL);
                double t;
                if (tab[nx + POL_MODE] != 0.0) { const double prev = vs[j]; t = policy_rule(tab, nx, xs, prev); sw += t != prev; }
                else t = uk[j];
                ws[nw + j] = t; vs[j] = t;
            }
        } else
            for (int j = lane; j < nu; j += SM_W) { const double t = uk[j]; ws[nw + j] = t; vs[j] = t; }
        sm_sync();
        if (M.n) {
            // ---- 2. the resolver's right-hand side: lanes on rows, j ascending
            for (int i = lane; i < m; i += SM_W) {
                double s = 0.0;
                for (int j = 0; j < nx; ++j) s += M.Hx[(size_t)i * nx + j] * xs[j];
                for (int j = 0; j < nw2; ++j) s += M.Hw[(size_t)i * nw2 + j] * ws[j];
                s += M.H5[i];
                hs[i] = M.rs[i] * s;
            }
            sm_sync();
            // ---- 3. delta, z, mu of least total slack
            [[maybe_unused]] int mk = RO_FIX_OPEN;
            if constexpr (FIX) mk = F->mark[k];      /* the same for every lane */
            if (FIX && mk == RO_FIX_NO_POINT) { end = RO_INFEASIBLE; break; }
            if (FIX && mk == RO_FIX_ANSWER) {
                for (int j = lane; j < M.n; j += SM_W) vs[nu + j] = F->ans[(size_t)k * M.n + j];
                sm_sync();
            } else {
                SmResult res;
                sm_solve(S, mem, A, lane, res);
                sm_sync();
                if (res.status != MLD_STATUS_OPTIMAL) {
                    end = res.status == MLD_STATUS_INFEASIBLE ? RO_INFEASIBLE : RO_DECLINED;
                    if constexpr (FIX) if (end == RO_DECLINED) {      /* the resolver's inputs of this step: x_k and omega' = [omega_k; u_k] */
                        for (int j = lane; j < nx; j += SM_W) F->ax0[j] = xs[j];
                        for (int j = lane; j < nw2; j += SM_W) F->aom[j] = ws[j];
                    }
                    break;
                }
            }
        }
        // ---- 4. x_{k+1}, y_k and the residuals: k_sim_step's, by the same functions (plant_step.inc)
        for (int i = lane; i < nx; i += SM_W) xn[i] = plant_row(i, P.b5, P.A, P.Bv, P.B4, nx, nv, nw, xs, vs, ws);
        for (int i = lane; i < ny; i += SM_W) {
            const double s = plant_row(i, P.d5, P.C, P.Dv, P.D4, nx, nv, nw, xs, vs, ws);
            ys[i] = s;
            if (T.y) T.y[(size_t)k * ny + i] = s;
        }
        sm_sync();
        double best = -S_INF; int brow = -1;
        for (int i = lane; i < nc; i += SM_W)
            plant_worst(plant_residual(i, P.E, P.Fv, P.F4, P.G, P.f5, nx, nv, nf, nw, ny, xs, vs, ws, ys), i, best, brow);
        for (int off = SM_W / 2; off; off >>= 1) plant_worst_merge(sm_xor_f64(best, off), sm_xor_i32(brow, off), best, brow);
        brow = sm_uniform(brow);
        // ---- 5. the reductions
        double pc = 0.0, pm = 0.0;
        for (int j = lane; j < nv; j += SM_W) {
            const double t = vs[j];
            if (T.cw) pc += T.cw[(size_t)k * nv + j] * t;
            if (j >= nf) pm += t;
        }
        if (T.cw) cost += sm_wave_sum(pc);
        mu_total += sm_wave_sum(pm);
        {
            const bool v_nan = best != best, w_nan = worst != worst;
            if (wstep < 0 || (!w_nan && (v_nan || best > worst))) { worst = best; wstep = k; wrow = brow; }      /* the earliest step of equals stays */
        }
        if constexpr (KPI) {      /* the record of step k is the staging: xs, vs, ys, ws[0 .. nw), xn (published by the barrier behind step 4) */
            const int nq = Q->n_kpi;
            const RoKpiAcc a = ro_kpi_acc(xn + nx, nq);
            const sm_f64 *const field[5] = {xs, vs, ys, ws, xn};
            const int width[5] = {nx, nv, ny, nw, nx};
            for (int q = lane; q < nq; q += SM_W) {
                double f = 0.0;
                int row = 0; bool first = true;
                for (int t = 0; t < 5; ++t) {
                    if (!(Q->given >> t & 1u)) continue;
                    f = ls_add_term(f, ls_dot(Q->W + (size_t)row * nq + q, (size_t)nq, field[t], width[t]), first);
                    first = false; row += width[t];
                }
                const int pc = Q->price_chan[q];
                if (pc >= 0) f = ls_priced(Q->price[(size_t)k * Q->n_chan + pc], f);
                LsAcc c;
                c.sum = a.sum[q]; c.min = a.min[q]; c.max = a.max[q]; c.prev = a.prev[q];
                c.min_step = a.steps[2 * q]; c.max_step = a.steps[2 * q + 1]; c.n_above = a.counts[2 * q]; c.n_changes = a.counts[2 * q + 1]; c.have_prev = k > 0;
                ls_accumulate(c, f, Q->thresh[q], k);
                a.sum[q] = c.sum; a.min[q] = c.min; a.max[q] = c.max; a.prev[q] = c.prev;
                a.steps[2 * q] = c.min_step; a.steps[2 * q + 1] = c.max_step; a.counts[2 * q] = c.n_above; a.counts[2 * q + 1] = c.n_changes;
            }
            n_vio += best > Q->vio_tol;      /* best is the wave's after the butterfly: every lane counts the same */
        }
        // ---- 6. what was asked for
        if (T.v) for (int j = lane; j < nv; j += SM_W) T.v[(size_t)k * nv + j] = vs[j];
        if (lane == 0) { if (T.vio) T.vio[k] = best; if (T.row) T.row[k] = brow; }
        sm_sync();
        for (int i = lane; i < nx; i += SM_W) { const double t = xn[i]; xs[i] = t; if (T.x) T.x[(size_t)(k + 1) * nx + i] = t; }
    }
    if (end != RO_COMPLETE) ro_blank(M, T, lane, k, false);
    R.end_status = end; R.steps_done = k;
    R.cost = end == RO_COMPLETE ? (T.cw ? cost : 0.0) : qnan; R.mu_total = end == RO_COMPLETE ? mu_total : qnan;
    R.worst_vio = end == RO_COMPLETE ? worst : qnan; R.worst_step = end == RO_COMPLETE ? wstep : -1; R.worst_row = end == RO_COMPLETE ? wrow : -1;
    if constexpr (POLICY) {
        for (int off = SM_W / 2; off; off >>= 1) sw += sm_xor_i32(sw, off);
        R.switches = end == RO_COMPLETE ? sm_uniform(sw) : -1;
    }
    if constexpr (KPI) ro_kpi_write(*Q, end == RO_COMPLETE ? xn + nx : nullptr, lane, n_vio);
    if constexpr (FIX) if (lane == 0) *F->step = end == RO_DECLINED ? k : -1;
}

#ifndef SM_HOST
struct RoDev {
    int batch, S, K;
    int nx, nu, nw, nv, nmu, ny, nc, m, n;
    int stage_doubles;
    const double *pack; size_t pack_len; PackOff off;      /* the models' packed blocks and the offsets inside one (mld_model_create) */
    const int *model_idx;
    const double *x0;                               /* (batch, nx): the handle's current state */
    const double *u; size_t u_stride, u_step;       /* the caller's (batch, K, nu): K nu, nu; the resident plan's rows: n, nv */
    const int *status; const double *obj;           /* the plan's, masking the instances without a usable one; nullptr = the caller's u */
    const double *om;                               /* (batch S, K nw) */
    const double *cw; int cw_by_inst;               /* (rows, K, nv), a row per model or per instance; nullptr = no cost */
    double *x, *v, *y, *vio; int *row;              /* per trajectory and step, any nullptr */
    double *cost, *mu_total, *worst_vio; int *worst_step, *steps_done, *end_status;      /* per trajectory, any nullptr */
    unsigned long long *counter;                    /* [0] the work queue, [1 .. 3] trajectories that ended complete / infeasible / declined */
};
struct RoPolicyDev {      /* what k_rollout_policy takes on top: an argument of its own, so that k_rollout's stay as they are */
    const double *tab; size_t tab_len;              /* (n_models, nu, nx + 5), tab_len = nu (nx + 5) */
    const double *u_prev;                           /* (batch, nu): the inputs before step 0 */
    int *switches;                                  /* per trajectory, or nullptr */
};

struct RoKpiDev {         /* what the KPI kernels take on top, likewise an argument of its own */
    int n_kpi, rows, n_chan, step;
    unsigned given;
    const double *W, *thresh; const int *price_chan;      /* (n_models, rows, n_kpi) KPI-minor, (n_models, n_kpi), (n_kpi) */
    const double *lib; const long long *price_start;      /* the resident price library and (batch) starts into it, or nullptr: no KPI is priced */
    double vio_tol;
    double *sum, *min, *max; int *min_step, *max_step, *n_above, *n_changes;      /* (batch S, n_kpi) */
    int *n_vio;                                           /* (batch S) */
};

struct RoCandDev {        /* what the candidate kernels take on top (mld_rollout_select), likewise an argument of its own */
    int P, plan_first;                              /* candidates per instance; candidate 0 is the resident plan (RoDev's u, u_stride, u_step, status, obj) */
    const double *u_cand;                           /* (batch, P - plan_first, K, nu): the other candidates */
};

struct RoCandPolDev {     /* what the candidate-policy kernels take on top (mld_rollout_select_policy), likewise an argument of its own */
    const double *tab; size_t tab_len;              /* (P - n_seq + 1, n_models, nu, nx + 5) in mld_upload_policy's row layout, tab_len = nu (nx + 5); the last table all mode 0 */
    int n_models, n_seq;                            /* candidates 0 .. n_seq - 1 are the plan and the sequences of u_cand (batch, n_seq - plan_first, K, nu) */
};

// The kernel body, written once and expanded into both kernels.  (A function template called by the two kernels was tried first: inlined, it left k_rollout
// with 208 bytes of scratch per lane instead of 156 -- the kernel arguments reach the register allocator by another route.  Expanded in place, the open-loop
// kernel's listing is the one it had: profiles/policy_rollout_resource_usage.txt.)  POLICY, KPI: literals; `pol`, `kd`: the kernel's RoPolicyDev and RoKpiDev (empty
// ones where the kernel takes none).  Flat KPI indices are 64-bit: t n_kpi over batch S trajectories.
// CAND (k_rollout_cand / k_rollout_cand_kpi, open loop only): P candidate input sequences per instance under the same S realisations -- trajectory
// t = (b P + p) S + c over a queue of batch P S; everything per instance is read at b, omega at b S + c (the buffer is laid out once for all candidates), every
// output at t.  Candidate 0 reads RoDev's u (the resident plan's rows, masked by plan_usable) where `plan_first` is set, the others read cd.u_cand; p, c and
// the two base addresses are computed once per trajectory, nothing else differs.  The four kernels without it expand RO_KERNEL_BODY as they always did.
// CAND and POLICY (k_rollout_cand_policy / k_rollout_cand_policy_kpi, mld_rollout_select_policy): the flag per trajectory is a TABLE per candidate -- M.pol is
// table ro_cand_table(cp) of `cq`, ruled for a policy candidate, all passed through for the plan and the sequences, whose rows of u_cand number n_seq -
// plan_first per instance; T.u of a policy candidate is u_cand's base, never read (every channel of it is ruled); u_prev is the instance's.  ro_run<true>
// is the one k_rollout_policy calls.
#define RO_KERNEL_BODY3(POLICY, KPI, CAND)                                                                                                                                \
    extern __shared__ double ro_lds[];                                                                                                                             \
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                                                                                    \
    sm_f64 *mem = (sm_f64 *)ro_lds + (size_t)wave * ((size_t)S.wave_doubles + a.stage_doubles), *stg = mem + S.wave_doubles;                                       \
    const unsigned long long total = CAND ? (unsigned long long)a.batch * cd.P * a.S : (unsigned long long)a.batch * a.S;                                          \
    RoModel M;                                                                                                                                                     \
    M.nx = a.nx; M.nu = a.nu; M.nw = a.nw; M.nv = a.nv; M.nmu = a.nmu; M.ny = a.ny; M.nc = a.nc; M.m = a.m; M.n = a.n;                                             \
    for (;;) {                                                                                                                                                     \
        const unsigned long long t = sm_claim(a.counter, lane);                                                                                                    \
        if (t >= total) break;                                                                                                                                     \
        const long long b = CAND ? (long long)(t / ((unsigned long long)cd.P * (unsigned)a.S)) : (long long)(t / (unsigned)a.S);                                   \
        [[maybe_unused]] int cp = 0;                                  /* CAND: the candidate, and the row of omega, b S + c */                                     \
        [[maybe_unused]] unsigned long long tw = t;                                                                                                                \
        if constexpr (CAND) {                                                                                                                                      \
            const unsigned long long r = t - (unsigned long long)b * cd.P * a.S;                                                                                   \
            cp = (int)(r / (unsigned)a.S);                                                                                                                         \
            tw = (unsigned long long)b * a.S + (r - (unsigned long long)cp * a.S);                                                                                 \
        }                                                                                                                                                          \
        [[maybe_unused]] const bool cand_plan = CAND && cd.plan_first && cp == 0;                                                                                  \
        const int mdl = a.model_idx ? a.model_idx[b] : 0;                                                                                                          \
        M.P = plant_mats(a.pack + (size_t)mdl * a.pack_len, a.off);                                                                                                \
        SmArgs A{};                                                                                                                                                \
        if (a.n) {                                                                                                                                                 \
            const size_t m = a.m, n = a.n;                                                                                                                         \
            M.Hx = P.Hx + (size_t)mdl * m * a.nx; M.Hw = P.Hw + (size_t)mdl * m * (a.nw + a.nu); M.H5 = P.H5 + (size_t)mdl * m; M.rs = P.rs + (size_t)mdl * m;     \
            A.G = P.Gs + (size_t)mdl * m * n; A.q = P.qs + (size_t)mdl * n;                                                                                        \
            A.lb = P.lb + (size_t)mdl * n; A.ub = P.ub + (size_t)mdl * n; A.cs = P.cs + (size_t)mdl * n;                                                           \
            A.is_int = P.is_int; A.bins = P.bins;                                                                                                                  \
        }                                                                                                                                                          \
        RoTraj T;                                                                                                                                                  \
        T.K = a.K; T.x0 = a.x0 + (size_t)b * a.nx; T.u = a.u + (size_t)b * a.u_stride; T.u_step = a.u_step;                                                        \
        if constexpr (CAND && !POLICY) if (!cand_plan) { T.u = cd.u_cand + ((size_t)b * (cd.P - cd.plan_first) + (cp - cd.plan_first)) * a.K * a.nu; T.u_step = (size_t)a.nu; }\
        if constexpr (CAND && POLICY) if (!cand_plan) {                                                                                                            \
            const bool seq = cp < cq.n_seq;                                                                                                                        \
            T.u = seq ? cd.u_cand + ((size_t)b * (cq.n_seq - cd.plan_first) + (cp - cd.plan_first)) * a.K * a.nu : cd.u_cand;                                      \
            T.u_step = seq ? (size_t)a.nu : 0;                                                                                                                     \
        }                                                                                                                                                          \
        T.om = a.om + (size_t)(CAND ? tw : t) * a.K * a.nw;                                                                                                        \
        T.cw = a.cw ? a.cw + (size_t)(a.cw_by_inst ? b : mdl) * a.K * a.nv : nullptr;                                                                              \
        T.x = a.x ? a.x + (size_t)t * (a.K + 1) * a.nx : nullptr; T.v = a.v ? a.v + (size_t)t * a.K * a.nv : nullptr;                                              \
        T.y = a.y ? a.y + (size_t)t * a.K * a.ny : nullptr; T.vio = a.vio ? a.vio + (size_t)t * a.K : nullptr; T.row = a.row ? a.row + (size_t)t * a.K : nullptr;  \
        if constexpr (POLICY) { M.pol = pol.tab + (size_t)mdl * pol.tab_len; T.u_prev = pol.u_prev + (size_t)b * a.nu; }                                           \
        if constexpr (POLICY && CAND) M.pol = ro_cand_rows(cq.tab, cq.tab_len, cq.n_models, cp, cq.n_seq, cd.P, mdl);                                              \
        [[maybe_unused]] RoKpi Q;                                                                                                                                  \
        if constexpr (KPI) {                                                                                                                                       \
            const size_t o = (size_t)t * (size_t)kd.n_kpi;                                                                                                         \
            Q.n_kpi = kd.n_kpi; Q.n_chan = kd.n_chan; Q.given = kd.given; Q.vio_tol = kd.vio_tol;                                                                  \
            Q.W = kd.W + (size_t)mdl * kd.rows * kd.n_kpi; Q.thresh = kd.thresh + (size_t)mdl * kd.n_kpi; Q.price_chan = kd.price_chan;                            \
            Q.price = kd.lib ? kd.lib + kd.price_start[b] + (long long)kd.step * kd.n_chan : nullptr;                                                              \
            Q.sum = kd.sum + o; Q.min = kd.min + o; Q.max = kd.max + o; Q.min_step = kd.min_step + o; Q.max_step = kd.max_step + o;                                \
            Q.n_above = kd.n_above + o; Q.n_changes = kd.n_changes + o; Q.n_vio = kd.n_vio + t;                                                                    \
        }                                                                                                                                                          \
        RoResult R;                                                                                                                                                \
        if ((!CAND || cand_plan) && a.status && !plan_usable(a.status, a.obj, (int)b)) {      /* uniform over the wave: no plan whose inputs could be applied */   \
            const double qnan = __builtin_nan("");                                                                                                                 \
            ro_blank(M, T, lane, 0, true);                                                                                                                         \
            R.cost = R.mu_total = R.worst_vio = qnan; R.worst_step = R.worst_row = -1; R.steps_done = 0; R.end_status = RO_NOT_ATTEMPTED;                          \
            if constexpr (POLICY) R.switches = -1;                                                                                                                 \
            if constexpr (KPI) ro_kpi_write(Q, nullptr, lane, 0);                                                                                                  \
        } else                                                                                                                                                     \
            ro_run<POLICY, KPI>(S, M, mem, stg, A, T, lane, R, KPI ? &Q : nullptr);                                                                                \
        if (lane == 0) {                                                                                                                                           \
            if (a.cost) a.cost[t] = R.cost;                                                                                                                        \
            if (a.mu_total) a.mu_total[t] = R.mu_total;                                                                                                            \
            if (a.worst_vio) a.worst_vio[t] = R.worst_vio;                                                                                                         \
            if (a.worst_step) a.worst_step[t] = R.worst_step;                                                                                                      \
            if (a.steps_done) a.steps_done[t] = R.steps_done;                                                                                                      \
            if (a.end_status) a.end_status[t] = R.end_status;                                                                                                      \
            if constexpr (POLICY) if (pol.switches) pol.switches[t] = R.switches;                                                                                  \
            if (R.end_status >= 0) atomicAdd(a.counter + 1 + R.end_status, 1ull);                                                                                  \
        }                                                                                                                                                          \
    }

// Three waves per SIMD asked for: unconstrained the kernel holds 219 VGPRs (two waves) and takes 1.44 x the time; at 168 it spills 42 registers to
// scratch, outside the pivot loop's hot values (DESIGN section 6).
#define RO_KERNEL_BODY(POLICY, KPI) const RoCandDev cd{}; const RoCandPolDev cq{}; RO_KERNEL_BODY3(POLICY, KPI, false)
__global__ void __launch_bounds__(SM_NT, 3) k_rollout(SmShape S, ProblemDev P, RoDev a)
{
    const RoPolicyDev pol{};
    const RoKpiDev kd{};
    RO_KERNEL_BODY(false, false)
}

// The policy instantiation: the same body, step 1's inputs by the rule.
__global__ void __launch_bounds__(SM_NT, 3) k_rollout_policy(SmShape S, ProblemDev P, RoDev a, RoPolicyDev pol)
{
    const RoKpiDev kd{};
    RO_KERNEL_BODY(true, false)
}

// The KPI instantiations (mld_rollout_kpi): the same body twice more, the trajectory's column statistics reduced in step 5.
__global__ void __launch_bounds__(SM_NT, 3) k_rollout_kpi(SmShape S, ProblemDev P, RoDev a, RoKpiDev kd)
{
    const RoPolicyDev pol{};
    RO_KERNEL_BODY(false, true)
}

__global__ void __launch_bounds__(SM_NT, 3) k_rollout_policy_kpi(SmShape S, ProblemDev P, RoDev a, RoPolicyDev pol, RoKpiDev kd)
{
    RO_KERNEL_BODY(true, true)
}

// The candidate instantiations (mld_rollout_select): the open-loop body twice more, P candidates per instance under the same realisations.
__global__ void __launch_bounds__(SM_NT, 3) k_rollout_cand(SmShape S, ProblemDev P, RoDev a, RoCandDev cd)
{
    const RoPolicyDev pol{};
    const RoKpiDev kd{};
    const RoCandPolDev cq{};
    RO_KERNEL_BODY3(false, false, true)
}

__global__ void __launch_bounds__(SM_NT, 3) k_rollout_cand_kpi(SmShape S, ProblemDev P, RoDev a, RoCandDev cd, RoKpiDev kd)
{
    const RoPolicyDev pol{};
    const RoCandPolDev cq{};
    RO_KERNEL_BODY3(false, true, true)
}

// The candidate-policy instantiations (mld_rollout_select_policy): the policy body twice more, a table per candidate.  Of `pol` they read u_prev and
// switches; the tables are cq's.
__global__ void __launch_bounds__(SM_NT, 3) k_rollout_cand_policy(SmShape S, ProblemDev P, RoDev a, RoCandDev cd, RoPolicyDev pol, RoCandPolDev cq)
{
    const RoKpiDev kd{};
    RO_KERNEL_BODY3(true, false, true)
}

__global__ void __launch_bounds__(SM_NT, 3) k_rollout_cand_policy_kpi(SmShape S, ProblemDev P, RoDev a, RoCandDev cd, RoPolicyDev pol, RoCandPolDev cq, RoKpiDev kd)
{
    RO_KERNEL_BODY3(true, true, true)
}
#undef RO_KERNEL_BODY
#undef RO_KERNEL_BODY3

// ---- the device completion's kernels (THE RULE: the header) ---------------------------------------------------------------------------------------------------
struct RoFixDev {
    long long n_items;                              /* listed trajectories this launch re-runs */
    const int *ent, *slot;                          /* (n_items): the entry e of the call's list, and its slot of the resolver's input buffers */
    const long long *list;                          /* (entries): the trajectory t of entry e */
    const double *ans; const int *mark;             /* (entries, K, n), (entries, K) */
    double *ax0, *aom;                              /* the resolver's inputs (slots, nx), (slots, nw + nu) */
    int *step;                                      /* (entries) */
    int sel;                                        /* the call is a selection: candidates other than the plan read u_cand */
};

// The list of the trajectories that ended 2, in any order: n[0] counts them (64-bit), entries past `cap` are counted and not written.
__global__ void __launch_bounds__(256) k_ro_collect(long long total, const int *end_status, long long cap, long long *list, unsigned long long *n)
{
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256)
        if (end_status[t] == RO_DECLINED) {
            const unsigned long long at = atomicAdd(n, 1ull);
            if (at < (unsigned long long)cap) list[at] = t;
        }
}

// The superset body over a LIST: a wave per item, t -> (b, p, c) as RO_KERNEL_BODY3 maps it (a call without candidates has P = 1), every output at t into
// the arrays of the first kernel.  A trajectory that now ends 0 or 1 is counted there (counter[1], counter[2]); counter[3] keeps what the first kernel declined.
template <bool KPI>
__device__ __forceinline__ void ro_redo_body(const SmShape &S, const ProblemDev &P, const RoDev &a, const RoCandDev &cd, const RoPolicyDev &pol, const RoCandPolDev &cq,
                                             const RoKpiDev &kd, const RoFixDev &fx)
{
    extern __shared__ double ro_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    sm_f64 *mem = (sm_f64 *)ro_lds + (size_t)wave * ((size_t)S.wave_doubles + a.stage_doubles), *stg = mem + S.wave_doubles;
    RoModel M;
    M.nx = a.nx; M.nu = a.nu; M.nw = a.nw; M.nv = a.nv; M.nmu = a.nmu; M.ny = a.ny; M.nc = a.nc; M.m = a.m; M.n = a.n;
    for (long long it = (long long)blockIdx.x * SM_WAVES + wave; it < fx.n_items; it += (long long)gridDim.x * SM_WAVES) {
        const size_t e = (size_t)fx.ent[it], sl = (size_t)fx.slot[it];
        const unsigned long long t = (unsigned long long)fx.list[e];
        const long long b = (long long)(t / ((unsigned long long)cd.P * (unsigned)a.S));
        const unsigned long long r = t - (unsigned long long)b * cd.P * a.S;
        const int cp = (int)(r / (unsigned)a.S);
        const unsigned long long tw = (unsigned long long)b * a.S + (r - (unsigned long long)cp * a.S);
        const bool cand_plan = fx.sel && cd.plan_first && cp == 0;
        const int mdl = a.model_idx ? a.model_idx[b] : 0;
        M.P = plant_mats(a.pack + (size_t)mdl * a.pack_len, a.off);
        SmArgs A{};
        if (a.n) {
            const size_t m = a.m, n = a.n;
            M.Hx = P.Hx + (size_t)mdl * m * a.nx; M.Hw = P.Hw + (size_t)mdl * m * (a.nw + a.nu); M.H5 = P.H5 + (size_t)mdl * m; M.rs = P.rs + (size_t)mdl * m;
            A.G = P.Gs + (size_t)mdl * m * n; A.q = P.qs + (size_t)mdl * n;
            A.lb = P.lb + (size_t)mdl * n; A.ub = P.ub + (size_t)mdl * n; A.cs = P.cs + (size_t)mdl * n;
            A.is_int = P.is_int; A.bins = P.bins;
        }
        RoTraj T;
        T.K = a.K; T.x0 = a.x0 + (size_t)b * a.nx; T.u = a.u + (size_t)b * a.u_stride; T.u_step = a.u_step;
        if (fx.sel && !cand_plan) {
            const bool seq = cp < cq.n_seq;
            T.u = seq ? cd.u_cand + ((size_t)b * (cq.n_seq - cd.plan_first) + (cp - cd.plan_first)) * a.K * a.nu : cd.u_cand;
            T.u_step = seq ? (size_t)a.nu : 0;
        }
        T.om = a.om + (size_t)tw * a.K * a.nw;
        T.cw = a.cw ? a.cw + (size_t)(a.cw_by_inst ? b : mdl) * a.K * a.nv : nullptr;
        T.x = a.x ? a.x + (size_t)t * (a.K + 1) * a.nx : nullptr; T.v = a.v ? a.v + (size_t)t * a.K * a.nv : nullptr;
        T.y = a.y ? a.y + (size_t)t * a.K * a.ny : nullptr; T.vio = a.vio ? a.vio + (size_t)t * a.K : nullptr; T.row = a.row ? a.row + (size_t)t * a.K : nullptr;
        M.pol = ro_cand_rows(cq.tab, cq.tab_len, cq.n_models, cp, cq.n_seq, cd.P, mdl);
        T.u_prev = pol.u_prev ? pol.u_prev + (size_t)b * a.nu : M.pol;      /* open loop: never used (every channel passed through), a valid address of nu doubles */
        [[maybe_unused]] RoKpi Q;
        if constexpr (KPI) {
            const size_t o = (size_t)t * (size_t)kd.n_kpi;
            Q.n_kpi = kd.n_kpi; Q.n_chan = kd.n_chan; Q.given = kd.given; Q.vio_tol = kd.vio_tol;
            Q.W = kd.W + (size_t)mdl * kd.rows * kd.n_kpi; Q.thresh = kd.thresh + (size_t)mdl * kd.n_kpi; Q.price_chan = kd.price_chan;
            Q.price = kd.lib ? kd.lib + kd.price_start[b] + (long long)kd.step * kd.n_chan : nullptr;
            Q.sum = kd.sum + o; Q.min = kd.min + o; Q.max = kd.max + o; Q.min_step = kd.min_step + o; Q.max_step = kd.max_step + o;
            Q.n_above = kd.n_above + o; Q.n_changes = kd.n_changes + o; Q.n_vio = kd.n_vio + t;
        }
        RoFix F;
        F.ans = fx.ans + e * (size_t)a.K * (size_t)a.n; F.mark = fx.mark + e * (size_t)a.K;
        F.ax0 = fx.ax0 + sl * (size_t)a.nx; F.aom = fx.aom + sl * (size_t)(a.nw + a.nu); F.step = fx.step + e;
        RoResult R;
        ro_run<true, KPI, true>(S, M, mem, stg, A, T, lane, R, KPI ? &Q : nullptr, &F);
        if (lane == 0) {
            if (a.cost) a.cost[t] = R.cost;
            if (a.mu_total) a.mu_total[t] = R.mu_total;
            if (a.worst_vio) a.worst_vio[t] = R.worst_vio;
            if (a.worst_step) a.worst_step[t] = R.worst_step;
            if (a.steps_done) a.steps_done[t] = R.steps_done;
            if (a.end_status) a.end_status[t] = R.end_status;
            if (pol.switches) pol.switches[t] = R.switches;
            if (R.end_status != RO_DECLINED) atomicAdd(a.counter + 1 + R.end_status, 1ull);
        }
    }
}
__global__ void __launch_bounds__(SM_NT) k_rollout_redo(SmShape S, ProblemDev P, RoDev a, RoCandDev cd, RoPolicyDev pol, RoCandPolDev cq, RoFixDev fx)
{
    const RoKpiDev kd{};
    ro_redo_body<false>(S, P, a, cd, pol, cq, kd, fx);
}
__global__ void __launch_bounds__(SM_NT) k_rollout_redo_kpi(SmShape S, ProblemDev P, RoDev a, RoCandDev cd, RoPolicyDev pol, RoCandPolDev cq, RoKpiDev kd, RoFixDev fx)
{
    ro_redo_body<true>(S, P, a, cd, pol, cq, kd, fx);
}

// The dense answer of slot[it] becomes entry (e, step[e]) of the table: usable -- status 0 or 2 with a finite objective (plan_usable) and finite values -- or
// "no feasible point".  A wave per item, lanes on the n values; an item whose trajectory ended in this round (step -1) has nothing to merge.
__global__ void __launch_bounds__(64) k_ro_fix_merge(long long n_items, const int *ent, const int *slot, const int *step, int K, int n, const double *aux_v, size_t aux_stride,
                                                     const int *aux_status, const double *aux_obj, double *ans, int *mark)
{
    const int lane = threadIdx.x;
    for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {
        const size_t e = (size_t)ent[it];
        const int k = step[e], sl = slot[it];
        if (k < 0 || k >= K) continue;
        bool ok = plan_usable(aux_status, aux_obj, sl);
        double *dst = ans + (e * (size_t)K + (size_t)k) * (size_t)n;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const double t = j < n ? aux_v[(size_t)sl * aux_stride + j] : 0.0;
            if (j < n) dst[j] = t;
            ok = __all(fabs(t) < __builtin_huge_val()) && ok;      /* (a NaN fails the comparison too) */
        }
        if (lane == 0) mark[e * (size_t)K + (size_t)k] = ok ? RO_FIX_ANSWER : RO_FIX_NO_POINT;
    }
}

// k_policy_inputs (mld_sim_step_policy): u[b, j] of ONE step for every instance, written into the buffer the resolving step reads its u0 from.  A ruled
// channel takes the rule's value from the handle's current x0[b] and the resident u_prev[b]; a passed-through one keeps the caller's value (src ==
// nullptr: already in u) or takes the resident plan's (src = the plan's rows, stride src_stride).  Threads on (instance, channel), 64-bit indices,
// grid-stride.
struct PolicyInputsArgs {
    long long batch; int nx, nu;
    const int *model_idx;
    const double *tab; size_t tab_len;
    const double *x0, *u_prev;                      /* (batch, nx), (batch, nu) */
    const double *src; size_t src_stride;           /* the passed-through channels where the caller brought none */
    double *u;                                      /* (batch, nu) */
};
__global__ void __launch_bounds__(256) k_policy_inputs(const PolicyInputsArgs a)
{
    const long long total = a.batch * a.nu;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long b = e / a.nu;
        const int j = (int)(e - b * a.nu);
        const double *tab = a.tab + (size_t)(a.model_idx ? a.model_idx[b] : 0) * a.tab_len + (size_t)j * (a.nx + POL_TAIL);
        if (tab[a.nx + POL_MODE] != 0.0) a.u[e] = policy_rule(tab, a.nx, a.x0 + b * a.nx, a.u_prev[e]);
        else if (a.src) a.u[e] = a.src[b * (long long)a.src_stride + j];
    }
}

// After an advancing step: the resident u_prev of every ADVANCED instance becomes the u applied (usable: k_aux_merge's flag, the mask k_sim_step advanced by).
__global__ void __launch_bounds__(256) k_policy_commit(long long batch, int nu, const unsigned char *usable, const double *u, double *u_prev)
{
    const long long total = batch * nu;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256)
        if (usable[e / nu]) u_prev[e] = u[e];
}
#endif
