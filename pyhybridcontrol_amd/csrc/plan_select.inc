// Plan selection: choose among P candidate input sequences per instance by their rollout risk (mld_rollout_select, api_rollout.inc).  A scenario-based
// controller rolls out several plans -- the one just solved, the shifted previous one, a baseline's nominal sequence -- under the same S realisations and
// applies the one whose risk is acceptable and whose cost is lowest; the same step is the safety filter in front of the plant step.  The candidates are rolled
// out by k_rollout_cand / k_rollout_cand_kpi (rollout.inc), trajectory t = (b P + p) S + c, their risk is k_rollout_risk's (rollout_risk.inc, unchanged) for
// "instance" i = b P + p, and this file holds what acts on it.
//
// THE RULE.  A STATISTIC is the triple (column j, kind, level index l) over the risk arrays of one candidate:
//     kind 0 mean[j]   1 min[j]   2 max[j]   3 (double)n_exceed[j]   4 quantile[j, l]   5 cvar_hi[j, l]   6 cvar_lo[j, l]          (l is read for 4 .. 6 only)
// Candidate p of instance b is ADMISSIBLE iff
//     counts[0] (its complete realisations) >= min_complete,
//     every constraint k < n_cons (at most MLD_SELECT_CONS_MAX): value(statistic k) <= bound[k] -- a NaN value fails --,
//     and its objective statistic is not NaN.
// The CHOICE is the admissible candidate that comes first in the order (value of the objective, p): a before a' iff v < v', or neither is smaller and p < p'
// (so a tie, and -0.0 against +0.0, goes to the smaller p) -- sel_before.  score = the chosen candidate's value; n_admissible counts; none admissible:
// choice -1, score NaN, the chosen inputs NaN.
//
// ARITHMETIC.  Comparisons only, and one int -> double conversion: nothing is rounded.  Written once as host-compilable functions (LS_FN), in the style of
// log_summary.inc and rollout_risk.inc: the device, scripts/plan_select_host_check.cpp and simlog.py: select_plan_np agree bit for bit.  The keys of two
// admissible candidates never tie (p is part of the key), so the arg-min does not depend on the order of the comparisons: the wave's butterfly gives the
// result of the serial scan.
//
// MAPPING of k_plan_select.  One 64-lane wave per instance, lane p = candidate p (P <= MLD_SELECT_P_MAX = 64), SEL_WAVES instances per workgroup, workgroups
// stride over the batch, the grid from the CU count (k_rollout_risk's mapping).  Lane p forms its statistics and its admissibility from the risk arrays, six
// xor steps carry the first key to every lane, lane 0 writes the per-instance outputs, and the wave's lanes copy the chosen sequence's K nu doubles -- the
// resident plan's strided rows or the candidate array -- into u_choice (and step 0 into u0_choice), lane-contiguous.  No LDS, no atomics, 64-bit flat
// indices, nothing checked here: the host has tested every argument before the launch.
#pragma once

#include "log_summary.inc"

enum { SEL_MEAN = 0, SEL_MIN, SEL_MAX, SEL_N_EXCEED, SEL_QUANTILE, SEL_CVAR_HI, SEL_CVAR_LO, SEL_N_KIND };
#define SEL_CONS_MAX 8      /* MLD_SELECT_CONS_MAX */

// One candidate's risk: (G) each, (G, L) for the per-level ones, counts (4).  An array no statistic of the call names may be null.
struct SelRisk {
    int L;
    const double *mean, *min, *max; const int *n_exceed;
    const double *quantile, *cvar_hi, *cvar_lo;
    const int *counts;
};
struct SelStat { int col, kind, lvl; };
// What a call selects by: the objective, the constraints and the least number of complete realisations
struct SelRule {
    SelStat obj;
    int n_cons;
    SelStat cons[SEL_CONS_MAX];
    double bound[SEL_CONS_MAX];
    int min_complete;
};

// the value of a statistic
LS_FN double sel_value(const SelRisk &R, const SelStat &s)
{
    const size_t o = (size_t)s.col * (size_t)R.L + (size_t)s.lvl;
    switch (s.kind) {
    case SEL_MEAN: return R.mean[s.col];
    case SEL_MIN: return R.min[s.col];
    case SEL_MAX: return R.max[s.col];
    case SEL_N_EXCEED: return (double)R.n_exceed[s.col];
    case SEL_QUANTILE: return R.quantile[o];
    case SEL_CVAR_HI: return R.cvar_hi[o];
    default: return R.cvar_lo[o];
    }
}

// is the candidate admissible?  score: its objective statistic (whatever the answer)
LS_FN bool sel_admissible(const SelRisk &R, const SelRule &rule, double &score)
{
    score = sel_value(R, rule.obj);
    bool ok = R.counts[0] >= rule.min_complete && !(score != score);
    for (int k = 0; k < rule.n_cons; ++k) ok = ok && sel_value(R, rule.cons[k]) <= rule.bound[k];      /* a NaN compares false */
    return ok;
}

// THE ORDER: does key (va, pa) come before key (vb, pb)?  p < 0: no candidate (it comes before nothing, and everything comes before it)
LS_FN bool sel_before(double va, int pa, double vb, int pb)
{
    if (pa < 0) return false;
    if (pb < 0) return true;
    if (va < vb) return true;
    if (vb < va) return false;
    return pa < pb;
}

// The serial scan: candidates 0 .. P - 1 with value v[p], admissible ok[p]; returns the choice (-1: none), score its value (NaN), n_adm the count
LS_FN int sel_scan(const double *v, const unsigned char *ok, int P, double &score, int &n_adm)
{
    int best = -1;
    double bv = __builtin_nan("");
    n_adm = 0;
    for (int p = 0; p < P; ++p) {
        if (!ok[p]) continue;
        ++n_adm;
        if (sel_before(v[p], p, bv, best)) { bv = v[p]; best = p; }
    }
    score = bv;
    return best;
}

// Where the chosen inputs of a call with policy candidates come from (k_select_inputs): the candidates are [plan (plan_first) | n_seq - plan_first rows of
// u_cand | the policies]; row = the pick's row among an instance's rows of u_cand (SEL_FROM_SEQ only).  Element e of the K nu chosen inputs of a policy
// pick: the rule's step 0 for e < nu, NaN behind it (sel_policy_row0).
enum { SEL_FROM_NONE = 0, SEL_FROM_PLAN, SEL_FROM_SEQ, SEL_FROM_POLICY };
LS_FN int sel_source(int pick, int plan_first, int n_seq, int &row)
{
    row = 0;
    if (pick < 0) return SEL_FROM_NONE;
    if (pick >= n_seq) return SEL_FROM_POLICY;
    if (plan_first && pick == 0) return SEL_FROM_PLAN;
    row = pick - (plan_first ? 1 : 0);
    return SEL_FROM_SEQ;
}
LS_FN bool sel_policy_row0(size_t e, size_t nu) { return e < nu; }

#if defined(__HIPCC__) && !defined(SM_HOST)
#include "rollout.inc"      /* policy_rule, ro_cand_table: k_select_inputs applies step 0 of ro_run<true> */
#define SEL_WAVES 4

struct SelArgs {
    int batch, P, G, L, K, nu, plan_first;
    SelRule rule;
    const double *mean, *min, *max; const int *n_exceed;                        /* (batch P, G) */
    const double *quantile, *cvar_hi, *cvar_lo;                                 /* (batch P, G, L) */
    const int *counts;                                                          /* (batch P, 4) */
    const double *plan; size_t plan_stride, plan_step;                          /* the resident plan's rows (candidate 0 with plan_first): n, nv */
    const double *u_cand;                                                       /* (batch, P - plan_first, K, nu) */
    int *choice; double *score; int *n_adm; unsigned char *adm;                 /* (batch) x 3, (batch, P); any nullptr */
    double *u_choice, *u0_choice;                                               /* (batch, K, nu), (batch, nu); any nullptr */
};

// The chosen sequence of instance b copied by its wave (k_plan_select, k_select_inputs): step k, input j at src[k step + j] -- the resident plan's strided rows
// or a row of the candidate array -- into u_choice[b] (K nu doubles) and step 0 into u0_choice[b]; src == nullptr (no choice): NaN.  Lane-contiguous stores.
__device__ __forceinline__ void sel_copy_inputs(const double *src, size_t step, int K, int nu_, long long b, int lane, double *u_choice, double *u0_choice)
{
    const size_t nu = (size_t)nu_, Knu = (size_t)K * nu;
    const double qnan = __builtin_nan("");
    if (u_choice)
        for (size_t e = lane; e < Knu; e += 64) {
            const size_t k = e / nu, j = e - k * nu;
            u_choice[(size_t)b * Knu + e] = src ? src[k * step + j] : qnan;
        }
    if (u0_choice)
        for (size_t j = lane; j < nu; j += 64) u0_choice[(size_t)b * nu + j] = src ? src[j] : qnan;
}

__global__ void __launch_bounds__(64 * SEL_WAVES) k_plan_select(const SelArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long batch = a.batch;
    const size_t G = (size_t)a.G, GL = G * (size_t)a.L, P = (size_t)a.P, Knu = (size_t)a.K * (size_t)a.nu;
    const double qnan = __builtin_nan("");
    for (long long b = (long long)blockIdx.x * SEL_WAVES + wave; b < batch; b += (long long)gridDim.x * SEL_WAVES) {      /* uniform over the wave */
        double v = qnan; int at = -1, ok = 0;
        if (lane < a.P) {
            const size_t i = (size_t)b * P + (size_t)lane;
            SelRisk R;
            R.L = a.L;
            R.mean = a.mean ? a.mean + i * G : nullptr; R.min = a.min ? a.min + i * G : nullptr; R.max = a.max ? a.max + i * G : nullptr;
            R.n_exceed = a.n_exceed ? a.n_exceed + i * G : nullptr;
            R.quantile = a.quantile ? a.quantile + i * GL : nullptr; R.cvar_hi = a.cvar_hi ? a.cvar_hi + i * GL : nullptr;
            R.cvar_lo = a.cvar_lo ? a.cvar_lo + i * GL : nullptr;
            R.counts = a.counts + i * 4;
            ok = sel_admissible(R, a.rule, v) ? 1 : 0;
            if (ok) at = lane;
            if (a.adm) a.adm[i] = (unsigned char)ok;
        }
        int n = ok;
        for (int o = 1; o < 64; o <<= 1) {      /* the butterfly: every lane ends with the first key of THE ORDER, and the count */
            const double v2 = __shfl_xor(v, o, 64);
            const int p2 = __shfl_xor(at, o, 64);
            if (sel_before(v2, p2, v, at)) { v = v2; at = p2; }
            n += __shfl_xor(n, o, 64);
        }
        const int pick = __builtin_amdgcn_readfirstlane(at);
        if (lane == 0) {
            if (a.choice) a.choice[b] = pick;
            if (a.score) a.score[b] = pick >= 0 ? v : qnan;
            if (a.n_adm) a.n_adm[b] = n;
        }
        /* the chosen sequence: step k, input j at src[k step + j] */
        const double *src = nullptr; size_t step = (size_t)a.nu;
        if (pick >= 0) {
            if (a.plan_first && pick == 0) { src = a.plan + (size_t)b * a.plan_stride; step = a.plan_step; }
            else src = a.u_cand + ((size_t)b * (size_t)(a.P - a.plan_first) + (size_t)(pick - a.plan_first)) * Knu;
        }
        sel_copy_inputs(src, step, a.K, a.nu, b, lane, a.u_choice, a.u0_choice);
    }
}

// k_select_inputs (mld_rollout_select_policy), queued behind k_plan_select: the chosen inputs where a candidate may be a closed-loop policy.  It reads
// choice[b].  A plan or sequence pick is copied by sel_copy_inputs, as k_plan_select copies it (the rows of u_cand number n_seq - plan_first per instance
// here).  A policy pick has no sequence -- its inputs differ from realisation to realisation -- but its step 0 does not: u0[b, j] = policy_rule(table of the
// pick, x0[b], u_prev[b, j]), the function and the operands of step 0 of ro_run<true>, so the same bits, and what the resolving plant step takes as u0; the
// row is also u[b, 0, :], and rows 1 .. K - 1 are NaN.  No choice: all NaN.  The mapping is k_plan_select's: one wave per instance, lane-contiguous stores,
// 64-bit flat indices, no LDS, no atomics.
struct SelInputsArgs {
    int batch, P, K, nu, nx, plan_first, n_seq, n_models;
    const int *choice;                                                          /* (batch): k_plan_select's */
    const double *plan; size_t plan_stride, plan_step;                          /* the resident plan's rows (candidate 0 with plan_first): n, nv */
    const double *u_cand;                                                       /* (batch, n_seq - plan_first, K, nu) */
    const double *tab; size_t tab_len;                                          /* RoCandPolDev's tables: (P - n_seq + 1, n_models, nu, nx + 5) */
    const int *model_idx; const double *x0, *u_prev;                            /* (batch) or nullptr, (batch, nx), (batch, nu) */
    double *u_choice, *u0_choice;                                               /* (batch, K, nu), (batch, nu); any nullptr */
};

__global__ void __launch_bounds__(64 * SEL_WAVES) k_select_inputs(const SelInputsArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long batch = a.batch;
    const size_t nu = (size_t)a.nu, Knu = (size_t)a.K * nu;
    const double qnan = __builtin_nan("");
    for (long long b = (long long)blockIdx.x * SEL_WAVES + wave; b < batch; b += (long long)gridDim.x * SEL_WAVES) {      /* uniform over the wave */
        const int pick = a.choice[b];
        int row;
        const int from = sel_source(pick, a.plan_first, a.n_seq, row);
        if (from == SEL_FROM_POLICY) {      /* the rule's step 0, lanes on channels; NaN behind it */
            const int mdl = a.model_idx ? a.model_idx[b] : 0;
            for (size_t e = lane; e < (a.u_choice ? Knu : nu); e += 64) {
                double t = qnan;
                if (sel_policy_row0(e, nu))
                    t = ro_cand_input(a.tab, a.tab_len, a.n_models, pick, a.n_seq, a.P, mdl, (int)e, a.nx, a.x0 + (size_t)b * (size_t)a.nx, a.u_prev[(size_t)b * nu + e]);
                if (a.u0_choice && e < nu) a.u0_choice[(size_t)b * nu + e] = t;
                if (a.u_choice) a.u_choice[(size_t)b * Knu + e] = t;
            }
            continue;
        }
        const double *src = nullptr; size_t step = nu;
        if (from == SEL_FROM_PLAN) { src = a.plan + (size_t)b * a.plan_stride; step = a.plan_step; }
        else if (from == SEL_FROM_SEQ) src = a.u_cand + ((size_t)b * (size_t)(a.n_seq - a.plan_first) + (size_t)row) * Knu;
        sel_copy_inputs(src, step, a.K, a.nu, b, lane, a.u_choice, a.u0_choice);
    }
}
#endif
