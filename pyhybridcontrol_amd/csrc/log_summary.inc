// Campaign KPIs: column statistics of the resident simulation log (mld_sim_log_summary, api_summary.inc).  The reference's result of a campaign is
// grid_sim_dataframe, and every figure its plotting scripts quote is a column statistic of that frame over time (examples/
// residential_mg_with_pv_and_dewhs/plotting/plot_multi_sim_campaign.py:69-131): cost.sum(axis=0), p_exp.sum(axis=0) with p_exp = y - z
// (modelling/micro_grid_agents.py:750-753), mu[..., 0].sum(axis=0) ...  The log lies in HBM, one array per field, each (cap, batch, width); the KPIs are a
// few dozen doubles per instance, so the reduction runs where the records are.
//
// THE RULE.  KPI q of model m is a linear functional of a record, given by up to five tables (n_models, n_kpi, width) over x, v, y, omega, x_k1:
//     s_t = sum_i w_t[m, q, i] * field_t[i]        i ascending, from 0.0                                   (ls_dot)
//     f   = s_x + s_v + s_y + s_omega + s_xk1      the GIVEN tables only, left to right from the first     (ls_add_term)
//     f   = price[k, b, c] * f                     where price_chan[q] = c >= 0: the armed stage cost's price record   (ls_priced)
// A record k counts for instance b -- is STEPPED -- if and only if x_k1[k, b, 0] is not NaN: k_sim_step's own marking of a skipped instance (sim_step.inc).
// Over the stepped records of [first, first + count), k ascending, per (b, q) (ls_accumulate):
//     sum += f (from 0.0);  min / min_step and max / max_step by strict < / >: the first attaining record wins, a NaN never wins, +inf / -inf / -1 when
//     empty;  n_above: records with f > thresh[m, q];  n_changes: stepped records whose f != the previous stepped record's f (a channel's switch count).
// Per instance (ls_fixed_accumulate): n_stepped; vio_max / vio_step of cons_vio by strict > (-inf / -1 when empty); n_vio: stepped records with
// cons_vio > vio_tol; and over ALL records of the range nodes_total (64-bit) and n_source[s]: records with u_source == s, s = 0, 1, 2.
//
// ARITHMETIC.  The rule is written ONCE as host-compilable functions (LS_FN) with contraction switched off: every product and every addition is rounded on
// its own, in the stated order, so the device, a stand-alone host program (scripts/log_summary_host_check.cpp) and the numpy restatement
// (pyhybridcontrol_amd/simlog.py: summary_np) agree bit for bit.
//
// MAPPING of k_log_summary: a read-once streaming reduction.  One 64-lane wave per instance, LS_WAVES instances per workgroup (neighbouring instances are
// contiguous in every field array), workgroups stride over the batch, the grid comes from the CU count.  Only the fields a given table reads are touched
// (and element 0 of x_k1, the marking).  A record's doubles are loaded by the lanes, one element each, into registers (LS_SLOTS per lane), parked in one of
// two LDS buffers of the wave, and the loads of record k + 1 are issued before record k is reduced: the loop carries a dependence only through the
// accumulators.  Lane q < n_kpi evaluates its functional from the staged copy (every lane reads the same address: a broadcast) against weights laid out
// (n_models, row, n_kpi) by the host, so that the lanes' weight loads are contiguous and stay in cache; its accumulators live in registers across k.  Lane
// 63 keeps the per-instance block.  Records wider than 64 * LS_SLOTS doubles are staged without the register prefetch (`prefetch` = 0): the same sums in
// the same order, so both paths agree bit for bit.  Flat indices are 64-bit (cap x batch x width passes 2^31 at 2 880 records of the cfg4 shard).  No
// atomics; nothing is checked here: the host has tested the range and every table before the launch.
#pragma once

#if defined(__HIPCC__)
#define LS_FN __host__ __device__ inline
#else
#define LS_FN static inline
#endif
#if defined(__clang__)
#define LS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define LS_NO_CONTRACT _Pragma("STDC FP_CONTRACT OFF")
#endif

// s = sum_i w[i * w_stride] * f[i], i ascending, from 0.0.  F: the field's element type -- double behind a generic pointer (k_log_summary, the host), or the
// rollout's LDS staging (sm_f64: ro_run's KPI variant, rollout.inc); the arithmetic is the same fp64 either way
template <typename F> LS_FN double ls_dot(const double *w, size_t w_stride, const F *f, int n)
{
    LS_NO_CONTRACT
    double s = 0.0;
    for (int i = 0; i < n; ++i) { const double t = w[(size_t)i * w_stride] * f[i]; s = s + t; }
    return s;
}

// f with the next given table's s added: the first given table starts the sum
LS_FN double ls_add_term(double f, double s, bool first)
{
    LS_NO_CONTRACT
    return first ? s : f + s;
}

LS_FN double ls_priced(double price, double f)
{
    LS_NO_CONTRACT
    return price * f;
}

// the functional of one record: w[t] the (m, q) row of table t or null (not given: no term at all), field[t] the record's field, width[t] its length;
// t = 0 .. 4: x, v, y, omega, x_k1
LS_FN double ls_functional(const double *const w[5], size_t w_stride, const double *const field[5], const int width[5])
{
    double f = 0.0;
    bool first = true;
    for (int t = 0; t < 5; ++t) {
        if (!w[t]) continue;
        f = ls_add_term(f, ls_dot(w[t], w_stride, field[t], width[t]), first);
        first = false;
    }
    return f;
}

// a record is stepped iff element 0 of its x_k1 is not NaN
LS_FN bool ls_stepped(double x_k1_0) { return !(x_k1_0 != x_k1_0); }

// 64-bit flat index of element e of record k, instance b in a (cap, batch, width) array
LS_FN size_t ls_index(long long k, long long batch, long long b, long long width, long long e)
{
    return (size_t)((k * batch + b) * width + e);
}

struct LsAcc {
    double sum, min, max, prev;
    int min_step, max_step, n_above, n_changes, have_prev;
};

LS_FN void ls_acc_init(LsAcc &a)
{
    a.sum = 0.0; a.min = (double)__builtin_inf(); a.max = -(double)__builtin_inf(); a.prev = 0.0;
    a.min_step = a.max_step = -1; a.n_above = a.n_changes = a.have_prev = 0;
}

// one STEPPED record k (absolute index) with the functional's value f
LS_FN void ls_accumulate(LsAcc &a, double f, double thresh, int k)
{
    LS_NO_CONTRACT
    a.sum = a.sum + f;
    if (f < a.min) { a.min = f; a.min_step = k; }
    if (f > a.max) { a.max = f; a.max_step = k; }
    if (f > thresh) a.n_above += 1;
    if (a.have_prev && f != a.prev) a.n_changes += 1;
    a.prev = f; a.have_prev = 1;
}

struct LsFixed {
    double vio_max;
    long long nodes_total;
    int n_stepped, vio_step, n_vio, n_source[3];
};

LS_FN void ls_fixed_init(LsFixed &a, bool has_source)
{
    a.vio_max = -(double)__builtin_inf(); a.nodes_total = 0; a.n_stepped = 0; a.vio_step = -1; a.n_vio = 0;
    a.n_source[0] = a.n_source[1] = a.n_source[2] = has_source ? 0 : -1;
}

// one record k of the range, stepped or not; source: its u_source (ignored when the log has no source array)
LS_FN void ls_fixed_accumulate(LsFixed &a, bool stepped, double vio, int nodes, int source, bool has_source, double vio_tol, int k)
{
    a.nodes_total += nodes;
    if (has_source) { a.n_source[0] += source == 0; a.n_source[1] += source == 1; a.n_source[2] += source == 2; }
    if (!stepped) return;
    a.n_stepped += 1;
    if (vio > a.vio_max) { a.vio_max = vio; a.vio_step = k; }
    if (vio > vio_tol) a.n_vio += 1;
}

#if defined(__HIPCC__)
#define LS_WAVES 4
#define LS_SLOTS 2                              /* registers a lane holds of the record in flight: records of up to 64 * LS_SLOTS doubles are prefetched */
#define LS_LDS_MAX ((size_t)48 << 10)           /* dynamic LDS of one workgroup the staging may use */
#define LS_SEG_MAX 6                            /* x, v, y, omega, x_k1, price */

/* one staged run of a record: `take` leading elements of a (cap, batch, width) array, parked at `off` in the wave's staging */
struct LsSeg { const double *base; int width, take, off; };

struct LogSummaryArgs {
    int batch, first, count, n_kpi, prefetch;
    int n_seg, n_fun;                           /* staged runs; the first n_fun of them are the given tables', in the order x, v, y, omega, x_k1 */
    int staged;                                 /* doubles staged per record */
    int flag_off, price_off;                    /* where x_k1[0] and the price record lie in the staging (price_off < 0: no KPI is priced) */
    int rows;                                   /* rows of W per model: the widths of the given tables */
    LsSeg seg[LS_SEG_MAX];
    const int *model_idx;
    const double *W;                            /* (n_models, rows, n_kpi): the given tables side by side, KPI-minor */
    const double *thresh; const int *price_chan;      /* (n_models, n_kpi), (n_kpi) */
    const double *vio; const int *nodes, *source;     /* (cap, batch) each; source may be null */
    double vio_tol;
    double *sum, *min, *max; int *min_step, *max_step, *n_above, *n_changes;      /* (batch, n_kpi) */
    int *n_stepped; double *vio_max; int *vio_step, *n_vio; long long *nodes_total; int *n_source;      /* (batch), n_source (batch, 3) */
};

/* the staged run that holds staged element j (a chain of selects: no run is indexed by a lane's value), and j's position in it */
__device__ inline LsSeg ls_seg_of(const LogSummaryArgs &a, int j, int &e)
{
    LsSeg g = a.seg[0];
#pragma unroll
    for (int s = 1; s < LS_SEG_MAX; ++s) if (s < a.n_seg && j >= a.seg[s].off) g = a.seg[s];
    e = j - g.off;
    return g;
}

__global__ void __launch_bounds__(64 * LS_WAVES) k_log_summary(const LogSummaryArgs a)
{
    extern __shared__ double ls_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = a.staged, Q = a.n_kpi;
    double *const stage = ls_lds + (size_t)wave * 2 * S;
    const long long batch = a.batch;
    for (long long base = (long long)blockIdx.x * LS_WAVES; base < batch; base += (long long)gridDim.x * LS_WAVES) {      /* uniform over the workgroup */
        const long long b = base + wave;
        const bool live = b < batch;
        const size_t m = (live && a.model_idx) ? (size_t)a.model_idx[b] : 0;
        /* this lane's elements of a record: where the first one lies, and how far the next record's is */
        const double *src[LS_SLOTS]; size_t hop[LS_SLOTS]; double reg[LS_SLOTS];
#pragma unroll
        for (int s = 0; s < LS_SLOTS; ++s) {
            const int j = lane + 64 * s;
            src[s] = nullptr; hop[s] = 0; reg[s] = 0.0;
            if (a.prefetch && live && j < S) {
                int e; const LsSeg g = ls_seg_of(a, j, e);
                src[s] = g.base + ls_index(a.first, batch, b, g.width, e);
                hop[s] = (size_t)batch * (size_t)g.width;
            }
        }
        const bool fixed_lane = live && lane == 63;
        const size_t rec0 = (size_t)a.first * (size_t)batch + (size_t)(live ? b : 0);
        double n_vio = 0.0; int n_nodes = 0, n_src = 0;      /* lane 63: the scalars of the record in flight */
        auto load_scalars = [&](size_t r) { n_vio = a.vio[r]; n_nodes = a.nodes[r]; n_src = a.source ? a.source[r] : 0; };
        LsAcc acc; ls_acc_init(acc);
        LsFixed fx; ls_fixed_init(fx, a.source != nullptr);
        const double thr = (live && lane < Q) ? a.thresh[m * Q + lane] : 0.0;
        const int pc = (lane < Q) ? a.price_chan[lane] : -1;
        const double *const wq = a.W + m * (size_t)a.rows * Q + (lane < Q ? lane : 0);
        if (a.count > 0) {
#pragma unroll
            for (int s = 0; s < LS_SLOTS; ++s) if (src[s]) reg[s] = *src[s];
            if (fixed_lane) load_scalars(rec0);
        }
        for (int kk = 0; kk < a.count; ++kk) {
            const int k = a.first + kk;
            double *const cur = stage + (size_t)(kk & 1) * S;
            const double c_vio = n_vio; const int c_nodes = n_nodes, c_src = n_src;
            if (a.prefetch) {
#pragma unroll
                for (int s = 0; s < LS_SLOTS; ++s) if (src[s]) { cur[lane + 64 * s] = reg[s]; src[s] += hop[s]; }
                if (kk + 1 < a.count) {      /* record k + 1 is in flight while record k is reduced */
#pragma unroll
                    for (int s = 0; s < LS_SLOTS; ++s) if (src[s]) reg[s] = *src[s];
                }
            } else if (live) {
                for (int j = lane; j < S; j += 64) {
                    int e; const LsSeg g = ls_seg_of(a, j, e);
                    cur[j] = g.base[ls_index(k, batch, b, g.width, e)];
                }
            }
            if (fixed_lane && kk + 1 < a.count) load_scalars(rec0 + (size_t)(kk + 1) * (size_t)batch);
            __syncthreads();      /* the staging of record k is written; two buffers: the one record k - 1 was read from is not touched before the next barrier */
            const bool stepped = live && ls_stepped(cur[a.flag_off]);
            if (stepped && lane < Q) {
                double f = 0.0;
                int row = 0;
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    if (t >= a.n_fun) break;
                    f = ls_add_term(f, ls_dot(wq + (size_t)row * Q, (size_t)Q, cur + a.seg[t].off, a.seg[t].take), t == 0);
                    row += a.seg[t].take;
                }
                if (pc >= 0) f = ls_priced(cur[a.price_off + pc], f);
                ls_accumulate(acc, f, thr, k);
            }
            if (fixed_lane) ls_fixed_accumulate(fx, stepped, c_vio, c_nodes, c_src, a.source != nullptr, a.vio_tol, k);
        }
        if (live && lane < Q) {
            const size_t o = (size_t)b * Q + lane;
            a.sum[o] = acc.sum; a.min[o] = acc.min; a.max[o] = acc.max;
            a.min_step[o] = acc.min_step; a.max_step[o] = acc.max_step; a.n_above[o] = acc.n_above; a.n_changes[o] = acc.n_changes;
        }
        if (fixed_lane) {
            a.n_stepped[b] = fx.n_stepped; a.vio_max[b] = fx.vio_max; a.vio_step[b] = fx.vio_step; a.n_vio[b] = fx.n_vio; a.nodes_total[b] = fx.nodes_total;
            for (int s = 0; s < 3; ++s) a.n_source[b * 3 + s] = fx.n_source[s];
        }
        __syncthreads();      /* the last record has been read before the next instance's first one is parked */
    }
}
#endif
