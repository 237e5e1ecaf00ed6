// Rollout risk: statistics ACROSS the realisations of a rollout (mld_rollout_risk, api_rollout.inc).  The reference's headline figures are a column statistic
// over time, ...sum(axis=0), followed by a reduction over the Monte-Carlo runs, .mean(level=[..., 'controller']) (examples/residential_mg_with_pv_and_dewhs/
// plotting/plot_multi_sim_campaign.py:69-131).  The first half is k_rollout's summaries and k_rollout_kpi's statistics, (batch, S) and (batch, S, n_kpi) in
// device temporaries of the call; this is the second half, reduced where those lie: a few doubles per (instance, column) instead of every trajectory's.
//
// THE RULE.  A call names G columns (1 .. MLD_RISK_COLS_MAX), column j = (src[j], q[j]):
//     src 0 cost, 1 mu_total, 2 worst_vio, 3 switches (policy only), 4 n_vio, 5 / 6 / 7 KPI sum / min / max of KPI q, 8 / 9 KPI n_above / n_changes of KPI q
// (integers become doubles exactly).  For instance b and column j, g[c] is realisation c's value; c is COMPLETE iff end_status[b, c] == 0; n = their number.
//   counts   per instance over all c: n_complete, n_infeasible (1), n_declined (2), n_not_attempted (-1)
//   order    the complete c ascending by (g, c): a before a' iff g < g', or g == g' and c < c' (-0.0 and +0.0 tie); a NaN after every number, by c
//            (risk_before; a stable sort by value).  sorted[r], r = 0 .. n - 1.
//   T        the balanced binary tree over 64 leaves in index order -- (0,1), (2,3), ... then those pairwise, six levels, every addition rounded on its
//            own; a leaf that is not selected is +0.0 (risk_tree).  The butterfly t[i] += t[i ^ 2^d] gives the same bits in every lane.
//   mean     T(leaf c = g[c] if complete) / n
//   min, min_c / max, max_c    by strict < / >, the smallest attaining c wins, a NaN never wins
//   n_exceed complete c with g[c] > level[j]
//   per level l, i = idx[l][n] (the host's rank table: the smallest i >= 0 with (double)(i + 1) >= alpha[l] * (double)n; risk_rank):
//   quantile = sorted[i], quantile_c its c;  cvar_hi = T(leaf r = sorted[r], i <= r < n) / (n - i);  cvar_lo = T(leaf r = sorted[r], r <= i) / (i + 1)
//   n == 0   mean, quantile, cvar_* NaN; min +inf, max -inf; every _c -1; n_exceed 0 (mld_sim_log_summary's conventions)
//
// ARITHMETIC.  Written once as host-compilable functions with contraction off (LS_NO_CONTRACT), in the style of log_summary.inc and of SM_HOST (small_lds.inc:
// a "wave" is one lane, LDS plain memory, the fences empty): the device, scripts/rollout_risk_host_check.cpp and simlog.py: rollout_risk_np agree bit for bit.
// The keys of a column are pairwise different (c is part of the key), so the sorted order does not depend on the network that produced it.
//
// MAPPING of k_rollout_risk.  One 64-lane wave per instance, lane c = realisation c (S <= MLD_RISK_S_MAX = 64), RISK_WAVES instances per workgroup, workgroups
// stride over the batch, the grid from the CU count (k_log_summary's mapping).  The waves share nothing: no __syncthreads, lanes hand values over through
// the wave's LDS between wavefront-scope fences (sm_sync).  An instance's S x n_kpi block of each KPI array is contiguous: the blocks of the arrays some
// column reads are staged into the wave's LDS with coalesced loads, each byte read once, at row stride n_kpi | 1 -- lane c reads element q of row c, and an
// odd stride (in doubles for ds_read_b64's 64 banks, in dwords for ds_read_b32's 32) puts the 32 lanes of a group on 32 different banks.  Then the columns
// are looped: keys into LDS, tree sum of the mean, a 64-key bitonic network over the indexed arrays (a lane per disjoint pair per stage, a fence between
// stages), and the order statistics read from the sorted arrays.  Blocks that do not fit the workgroup's LDS (RISK_LDS_MAX) are not staged: the columns then
// read the arrays in place (`staged` = 0), the same values and so the same bits.  64-bit flat indices, no atomics, nothing checked here: the host has tested
// every argument before the launch.
#pragma once

#include "small_lds.inc"
#include "log_summary.inc"

enum { RISK_COST = 0, RISK_MU_TOTAL, RISK_WORST_VIO, RISK_SWITCHES, RISK_N_VIO, RISK_KPI_SUM, RISK_KPI_MIN, RISK_KPI_MAX, RISK_KPI_N_ABOVE, RISK_KPI_N_CHANGES, RISK_N_SRC };
#define RISK_NAN_TAG 64        /* tag = c, + 64 for a NaN, + 128 for a realisation that is not complete: numbers, then NaNs, then the absent ones, each by c */
#define RISK_ABSENT_TAG 128
#define RISK_SORT_DOUBLES 160  /* a wave's sort region: 64 values, 64 leaves (doubles), 64 tags (ints) */

// The rank table's entry: the smallest i >= 0 with (double)(i + 1) >= alpha * (double)n -- the index ceil(alpha n) - 1.  alpha in (0, 1] gives i <= n - 1.
static inline int risk_rank(double alpha, int n)
{
    LS_NO_CONTRACT
    const double an = alpha * (double)n;
    int i = 0;
    while (i + 1 < n && !((double)(i + 1) >= an)) ++i;
    return i;
}

// THE ORDER: does key (ga, ta) come before key (gb, tb)?  tags as above; two keys never tie (their c differ)
LS_FN bool risk_before(double ga, int ta, double gb, int tb)
{
    if ((ta | tb) >= RISK_NAN_TAG) return ta < tb;
    if (ga < gb) return true;
    if (gb < ga) return false;
    return ta < tb;
}

// What the core reads for one instance: the S entries of each per-trajectory summary, and the instance's (S, n_kpi) blocks at row stride ld (staged copies or
// the arrays themselves).  A source no column names may be null.
struct RiskIn {
    int S, G, L, ld;
    const int *src, *q;                      // (G)
    const double *level;                     // (G) or null = +inf
    const int *idx;                          // (L, S): idx[l S + n - 1]
    const int *es;                           // end_status
    const double *cost, *mu, *wv; const int *sw, *nvio;
    const double *ksum, *kmin, *kmax; const int *kabove, *kchg;
};
// Where one instance's results go: (G) each, (G, L) for the per-level ones, counts (4).  Any may be null.
struct RiskOut {
    double *mean, *min, *max; int *min_c, *max_c, *n_exceed;
    double *quantile, *cvar_hi, *cvar_lo; int *quantile_c;
    int *counts;
};

// g[c] of column (src, q)
SM_FN double risk_value(const RiskIn &I, int src, int q, int c)
{
    const size_t e = (size_t)c * (size_t)I.ld + (size_t)q;
    switch (src) {
    case RISK_COST: return I.cost[c];
    case RISK_MU_TOTAL: return I.mu[c];
    case RISK_WORST_VIO: return I.wv[c];
    case RISK_SWITCHES: return (double)I.sw[c];
    case RISK_N_VIO: return (double)I.nvio[c];
    case RISK_KPI_SUM: return I.ksum[e];
    case RISK_KPI_MIN: return I.kmin[e];
    case RISK_KPI_MAX: return I.kmax[e];
    case RISK_KPI_N_ABOVE: return (double)I.kabove[e];
    default: return (double)I.kchg[e];
    }
}

// T of the 64 leaves in t (written and fenced by the caller), in every lane.  The host walks the tree level by level on a copy; the device's butterfly adds
// the same pairs (an addition does not depend on the order of its operands).  The caller fences before t is written again.
SM_FN double risk_tree(const sm_f64 *t, int lane)
{
    LS_NO_CONTRACT
#ifdef SM_HOST
    (void)lane;
    double w[64];
    for (int i = 0; i < 64; ++i) w[i] = t[i];
    for (int d = 1; d < 64; d <<= 1)
        for (int i = 0; i < 64; i += 2 * d) w[i] = w[i] + w[i + d];
    return w[0];
#else
    double v = t[lane];
    for (int d = 1; d < 64; d <<= 1) { const double o = sm_xor_f64(v, d); v = v + o; }
    return v;
#endif
}

// the lanes' partial counts added up, in every lane
SM_FN int risk_count(int v)
{
    for (int o = 1; o < SM_W; o <<= 1) v += sm_xor_i32(v, o);
    return v;
}
SM_FN int risk_least(int v)
{
    for (int o = 1; o < SM_W; o <<= 1) { const int w = sm_xor_i32(v, o); v = w < v ? w : v; }
    return v;
}

// The 64 keys (sv[i], st[i]) into THE ORDER: the bitonic network on the indexed arrays, stage (k, j) compares the disjoint pairs (i, i | j) with bit j of i
// clear, ascending where bit k of i is clear; a lane per pair, a fence between stages.  Only the first P keys are sorted, P the power of two that holds the S
// realisations: the keys behind them are absent realisations, which lie in their place already (tag 128 + c, ascending, behind every key before them).
SM_FN void risk_sort64(sm_f64 *sv, sm_i32 *st, int P, int lane)
{
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int pr = lane; pr < P / 2; pr += SM_W) {
                const int lo = ((pr & ~(j - 1)) << 1) | (pr & (j - 1)), hi = lo | j;
                const double ga = sv[lo], gb = sv[hi];
                const int ta = st[lo], tb = st[hi];
                const bool swap = (lo & k) == 0 ? risk_before(gb, tb, ga, ta) : risk_before(ga, ta, gb, tb);
                if (swap) { sv[lo] = gb; sv[hi] = ga; st[lo] = tb; st[hi] = ta; }
            }
            sm_sync();
        }
}

// One instance, every column.  sv, tt: 64 doubles each, st: 64 ints of the wave's LDS (exactly; the host check gives no more).
SM_FN void risk_instance(const RiskIn &I, const RiskOut &O, sm_f64 *sv, sm_f64 *tt, sm_i32 *st, int lane)
{
    LS_NO_CONTRACT
    const double qnan = __builtin_nan(""), inf = (double)__builtin_inf();
    const int S = I.S;
    int P = 1;
    while (P < S) P <<= 1;
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    for (int c = lane; c < S; c += SM_W) { const int e = I.es[c]; n0 += e == 0; n1 += e == 1; n2 += e == 2; n3 += e == -1; }
    const int n = risk_count(n0);
    n1 = risk_count(n1); n2 = risk_count(n2); n3 = risk_count(n3);
    if (O.counts && lane == 0) { O.counts[0] = n; O.counts[1] = n1; O.counts[2] = n2; O.counts[3] = n3; }
    for (int j = 0; j < I.G; ++j) {
        const int src = I.src[j], q = I.q[j];
        const double level = I.level ? I.level[j] : inf;
        /* the keys, and the leaves of the mean */
        int numbers = 0;
        for (int c = lane; c < 64; c += SM_W) {
            double g = 0.0; int tag = RISK_ABSENT_TAG + c;
            if (c < S && I.es[c] == 0) {
                g = risk_value(I, src, q, c);
                const bool nan = g != g;
                tag = c + (nan ? RISK_NAN_TAG : 0);
                numbers += !nan;
            }
            sv[c] = g; tt[c] = g; st[c] = tag;
        }
        const int m = risk_count(numbers);      /* the complete realisations whose value is a number: sorted[0 .. m) */
        sm_sync();
        const double total = risk_tree(tt, lane);
        risk_sort64(sv, st, P, lane);
        /* the extremes and the exceedances from the sorted keys: sorted[0] is the least number at its smallest c; the greatest is sorted[m - 1], and the
         * first of its equals carries the smallest c */
        const double top = m > 0 ? sv[m - 1] : -inf;
        int first_top = SM_NONE, above = 0;
        for (int r = lane; r < n; r += SM_W) {
            const double g = sv[r];
            if (r < m && g == top && r < first_top) first_top = r;
            above += g > level;
        }
        first_top = risk_least(first_top);
        above = risk_count(above);
        if (lane == 0) {
            if (O.mean) O.mean[j] = n > 0 ? total / (double)n : qnan;
            if (O.min) O.min[j] = m > 0 ? sv[0] : inf;
            if (O.min_c) O.min_c[j] = m > 0 ? st[0] : -1;
            if (O.max) O.max[j] = m > 0 ? sv[first_top] : -inf;      /* (the value at that c: the zeros tie, and their signs may differ) */
            if (O.max_c) O.max_c[j] = m > 0 ? st[first_top] : -1;
            if (O.n_exceed) O.n_exceed[j] = above;
        }
        for (int l = 0; l < I.L; ++l) {
            const size_t o = (size_t)j * (size_t)I.L + (size_t)l;
            if (n == 0) {
                if (lane == 0) {
                    if (O.quantile) O.quantile[o] = qnan;
                    if (O.quantile_c) O.quantile_c[o] = -1;
                    if (O.cvar_hi) O.cvar_hi[o] = qnan;
                    if (O.cvar_lo) O.cvar_lo[o] = qnan;
                }
                continue;
            }
            const int i = I.idx[(size_t)l * (size_t)S + (size_t)(n - 1)];
            sm_sync();
            for (int r = lane; r < 64; r += SM_W) tt[r] = (r >= i && r < n) ? sv[r] : 0.0;
            sm_sync();
            const double hi = risk_tree(tt, lane);
            sm_sync();
            for (int r = lane; r < 64; r += SM_W) tt[r] = r <= i ? sv[r] : 0.0;
            sm_sync();
            const double lo = risk_tree(tt, lane);
            if (lane == 0) {
                if (O.quantile) O.quantile[o] = sv[i];
                if (O.quantile_c) O.quantile_c[o] = st[i] & (RISK_NAN_TAG - 1);
                if (O.cvar_hi) O.cvar_hi[o] = hi / (double)(n - i);
                if (O.cvar_lo) O.cvar_lo[o] = lo / (double)(i + 1);
            }
        }
        sm_sync();      /* the sorted keys have been read before the next column's are written */
    }
}

#if defined(__HIPCC__) && !defined(SM_HOST)
#define RISK_WAVES 4
#define RISK_LDS_MAX ((size_t)64 << 10)      /* dynamic LDS of one workgroup: the sort regions and the staged blocks */

struct RiskArgs {
    int batch, S, G, L, n_kpi;
    int staged, ld;                             /* blocks staged at row stride ld = n_kpi | 1, or read in place at ld = n_kpi */
    unsigned need;                              /* bit t: some column reads KPI array t of sum, min, max, n_above, n_changes */
    int off[5];                                 /* where block t lies in the wave's staging, in doubles behind the sort region */
    int wave_doubles;                           /* doubles of LDS per wave */
    const int *col_src, *col_q; const double *level; const int *idx;
    const int *es; const double *cost, *mu, *wv; const int *sw, *nvio;                      /* (batch, S) */
    const double *ksum, *kmin, *kmax; const int *kabove, *kchg;                             /* (batch, S, n_kpi) */
    double *mean, *min, *max; int *min_c, *max_c, *n_exceed;                                /* (batch, G) */
    double *quantile, *cvar_hi, *cvar_lo; int *quantile_c;                                  /* (batch, G, L) */
    int *counts;                                                                            /* (batch, 4) */
};

/* doubles a wave stages: the blocks the columns read, doubles whole and ints two to a double, each rounded up to an even count */
static inline size_t risk_stage_doubles(int S, int n_kpi, unsigned need, int off[5])
{
    const size_t block = (size_t)S * (size_t)(n_kpi | 1);
    size_t at = 0;
    for (int t = 0; t < 5; ++t) {
        off[t] = (int)at;
        if (need >> t & 1u) at += t < 3 ? block : (block + 1) / 2;
        at = (at + 1) & ~(size_t)1;
    }
    return at;
}

template <typename T> __device__ inline const T *risk_stage(const T *block, sm_f64 *dst, bool take, int S, int n_kpi, int ld, int lane)
{
    if (!take) return nullptr;
    typedef __attribute__((address_space(3))) T lds_t;
    lds_t *const d = (lds_t *)dst;
    const int len = S * n_kpi;
    for (int e = lane; e < len; e += 64) d[(e / n_kpi) * ld + e % n_kpi] = block[e];
    return (const T *)d;
}

__global__ void __launch_bounds__(64 * RISK_WAVES) k_rollout_risk(const RiskArgs a)
{
    extern __shared__ double risk_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    sm_f64 *const mem = (sm_f64 *)risk_lds + (size_t)wave * (size_t)a.wave_doubles;
    sm_f64 *const sv = mem, *const tt = mem + 64, *const stg = mem + RISK_SORT_DOUBLES;
    sm_i32 *const st = (sm_i32 *)(mem + 128);
    const long long batch = a.batch;
    const size_t S = (size_t)a.S, Q = (size_t)a.n_kpi, G = (size_t)a.G, L = (size_t)a.L;
    for (long long b = (long long)blockIdx.x * RISK_WAVES + wave; b < batch; b += (long long)gridDim.x * RISK_WAVES) {      /* uniform over the wave */
        const size_t t0 = (size_t)b * S, k0 = t0 * Q, g0 = (size_t)b * G;
        RiskIn I;
        I.S = a.S; I.G = a.G; I.L = a.L; I.ld = a.ld;
        I.src = a.col_src; I.q = a.col_q; I.level = a.level; I.idx = a.idx;
        I.es = a.es + t0;
        I.cost = a.cost ? a.cost + t0 : nullptr; I.mu = a.mu ? a.mu + t0 : nullptr; I.wv = a.wv ? a.wv + t0 : nullptr;
        I.sw = a.sw ? a.sw + t0 : nullptr; I.nvio = a.nvio ? a.nvio + t0 : nullptr;
        if (a.staged) {
            I.ksum = risk_stage(a.ksum + k0, stg + a.off[0], a.need & 1u, a.S, a.n_kpi, a.ld, lane);
            I.kmin = risk_stage(a.kmin + k0, stg + a.off[1], a.need & 2u, a.S, a.n_kpi, a.ld, lane);
            I.kmax = risk_stage(a.kmax + k0, stg + a.off[2], a.need & 4u, a.S, a.n_kpi, a.ld, lane);
            I.kabove = risk_stage(a.kabove + k0, stg + a.off[3], a.need & 8u, a.S, a.n_kpi, a.ld, lane);
            I.kchg = risk_stage(a.kchg + k0, stg + a.off[4], a.need & 16u, a.S, a.n_kpi, a.ld, lane);
            sm_sync();
        } else {
            I.ksum = a.ksum ? a.ksum + k0 : nullptr; I.kmin = a.kmin ? a.kmin + k0 : nullptr; I.kmax = a.kmax ? a.kmax + k0 : nullptr;
            I.kabove = a.kabove ? a.kabove + k0 : nullptr; I.kchg = a.kchg ? a.kchg + k0 : nullptr;
        }
        RiskOut O;
        O.mean = a.mean ? a.mean + g0 : nullptr; O.min = a.min ? a.min + g0 : nullptr; O.max = a.max ? a.max + g0 : nullptr;
        O.min_c = a.min_c ? a.min_c + g0 : nullptr; O.max_c = a.max_c ? a.max_c + g0 : nullptr; O.n_exceed = a.n_exceed ? a.n_exceed + g0 : nullptr;
        O.quantile = a.quantile ? a.quantile + g0 * L : nullptr; O.cvar_hi = a.cvar_hi ? a.cvar_hi + g0 * L : nullptr;
        O.cvar_lo = a.cvar_lo ? a.cvar_lo + g0 * L : nullptr; O.quantile_c = a.quantile_c ? a.quantile_c + g0 * L : nullptr;
        O.counts = a.counts ? a.counts + (size_t)b * 4 : nullptr;
        risk_instance(I, O, sv, tt, st, lane);
        sm_sync();      /* the staged blocks have been read before the next instance's are parked */
    }
}
#endif
