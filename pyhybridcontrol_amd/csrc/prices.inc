// Resident price profiles (mld_upload_prices and its two consumers): every solve of the reference's closed loop starts from a price window and every plant
// step ends in a price --
//   get_price_tilde_k     price_profile.values[start:start + N_tilde]                     (modelling/micro_grid_agents.py:563-606)
//   sim_mpc               q_z = prices_tilde, q_mu = sum(prices_tilde) * P_h_Nom * mult    (micro_grid_control_simulation.py:186-198)
//   sim_step_k            cost = sim_k.z * prices_k                                        (micro_grid_agents.py:746-755)
// -- so the tariff is a flat library in HBM, a series row-major (time, n_chan), and a window is a start offset (the window rule of profiles.inc with ONE
// group of width n_chan):    price[k, c] = lib[s + (step + k) * n_chan + c]
//   k_price_cost   the linear weights of a resident batch from its price windows and small per-model tables, into the buffers mld_upload_instance_cost fills
//   k_stage_cost   price and stage cost of a simulation-log record, and the running total per instance
//
// ARITHMETIC.  Both formulas are written ONCE as host-compilable functions (PR_FN) with contraction switched off: every product and every addition is
// rounded on its own, in the stated order, so the device, a stand-alone host program and the numpy restatement (pyhybridcontrol_amd/prices.py) agree bit
// for bit.  (hipcc contracts a * b + c into one fused multiply-add by default.)
//
// Mapping of k_price_cost: the destination is the large side (151 MB at the cfg4 shard), the library and the tables are small and stay in cache.  One
// 64-lane wave per destination ROW (instance), PC_WAVES rows per workgroup, workgroups stride over the batch.  A window is contiguous in the library:
// the wave stages its N_tilde * n_chan doubles in LDS with one coalesced sweep, lanes c < n_chan form S[c] there (a serial sum by definition: one rounding
// per addition, k ascending), then the lanes stride over the row's elements -- a wave's 64 stores are 512 contiguous bytes, the flat index is 64-bit,
// the split into (step, column) 32-bit.  Nothing is checked here: the host has tested every start against the window rule before the launch.  No atomics.
#pragma once

#if defined(__HIPCC__)
#define PR_FN __host__ __device__ inline
#else
#define PR_FN static inline
#endif
#if defined(__clang__)
#define PR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PR_NO_CONTRACT _Pragma("STDC FP_CONTRACT OFF")
#endif

// S[c] = p[0, c] + p[1, c] + ... + p[N - 1, c]; win: the window (N, n_chan)
PR_FN double price_window_sum(const double *win, int N, int n_chan, int c)
{
    PR_NO_CONTRACT
    double S = win[c];
    for (int k = 1; k < N; ++k) S = S + win[(size_t)k * n_chan + c];
    return S;
}

// one weight of step k: sum_c a[c, j] * p[k, c]  +  sum_c s[c, j] * S[c].  a, s: one model's tables (n_chan, W), s may be null (no sum term: the weights
// on y); pk: the window's row k; S: the window's sums
PR_FN double price_cost_elem(const double *a, const double *s, const double *pk, const double *S, int n_chan, int W, int j)
{
    PR_NO_CONTRACT
    double acc = 0.0;
    for (int c = 0; c < n_chan; ++c) { const double t = a[(size_t)c * W + j] * pk[c]; acc = acc + t; }
    if (!s) return acc;
    double acs = 0.0;
    for (int c = 0; c < n_chan; ++c) { const double t = s[(size_t)c * W + j] * S[c]; acs = acs + t; }
    return acc + acs;
}

// the stage cost of one record: sum_c price[c] * ( sum_j w_v[c, j] v[j]  +  sum_j w_y[c, j] y[j] ).  w_v (n_chan, nv), w_y (n_chan, ny): one model's tables
PR_FN double stage_cost_value(const double *w_v, const double *w_y, const double *price, const double *v, const double *y, int n_chan, int nv, int ny)
{
    PR_NO_CONTRACT
    double cost = 0.0;
    for (int c = 0; c < n_chan; ++c) {
        double sv = 0.0, sy = 0.0;
        for (int j = 0; j < nv; ++j) { const double t = w_v[(size_t)c * nv + j] * v[j]; sv = sv + t; }
        for (int j = 0; j < ny; ++j) { const double t = w_y[(size_t)c * ny + j] * y[j]; sy = sy + t; }
        const double inner = sv + sy;
        const double t = price[c] * inner;
        cost = cost + t;
    }
    return cost;
}

#if defined(__HIPCC__)
#define PC_WAVES 4
#define PC_LDS_MAX ((size_t)48 << 10)      /* dynamic LDS of one workgroup the staging may use */

// doubles a wave stages per row: the window and its sums
PR_FN size_t price_stage_doubles(int N, int n_chan) { return ((size_t)N + 1) * (size_t)n_chan; }

struct PriceCostArgs {
    int batch, N, n_chan, W, rpw, step;             /* W: columns per step of this launch (nv or ny); rpw: rows per workgroup (1 .. PC_WAVES, by the LDS the staging needs) */
    const int *model_idx;
    const long long *start; const double *lib;      /* (batch) starts into the price library */
    const double *a, *s;                            /* (n_models, n_chan, W) each; s may be null */
    double *dst; size_t ld;                         /* row b begins at dst + b * ld; its first N * W entries are written */
};

__global__ void __launch_bounds__(64 * PC_WAVES) k_price_cost(const PriceCostArgs a)
{
    extern __shared__ double pc_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N, C = a.n_chan, W = a.W;
    double *const win = pc_lds + (size_t)wave * price_stage_doubles(N, C), *const S = win + (size_t)N * C;
    const unsigned row_len = (unsigned)N * (unsigned)W;
    for (long long base = (long long)blockIdx.x * a.rpw; base < a.batch; base += (long long)gridDim.x * a.rpw) {      /* uniform over the workgroup */
        const long long b = base + wave;
        const bool live = wave < a.rpw && b < a.batch;
        if (live) {
            const double *src = a.lib + a.start[b] + (long long)a.step * C;
            for (int i = lane; i < N * C; i += 64) win[i] = src[i];
        }
        __syncthreads();
        if (live && a.s) for (int c = lane; c < C; c += 64) S[c] = price_window_sum(win, N, C, c);
        __syncthreads();
        if (live) {
            const size_t tab = (size_t)(a.model_idx ? a.model_idx[b] : 0) * C * W;
            const double *ta = a.a + tab, *ts = a.s ? a.s + tab : nullptr;
            double *row = a.dst + (size_t)b * a.ld;
            for (unsigned e = lane; e < row_len; e += 64) {
                const unsigned k = e / (unsigned)W, j = e - k * (unsigned)W;
                row[e] = price_cost_elem(ta, ts, win + (size_t)k * C, S, C, W, (int)j);
            }
        }
        __syncthreads();      /* the row has read the staging before the next one overwrites it */
    }
}

// Price and stage cost of the record a step has just written (launched behind k_sim_step on the same stream): one thread per instance -- the sums are
// serial by definition and nv + ny is a few dozen; the record's v and y rows are read where k_sim_step left them.  `usable` is k_sim_step's own rule.
struct StageCostArgs {
    int batch, n_chan, nv, ny, step;
    const int *model_idx;
    const unsigned char *mask; const int *status; const double *obj;      /* as SimStepArgs: who was stepped */
    const long long *start; const double *lib;
    const double *w_v, *w_y;                        /* (n_models, n_chan, nv), (n_models, n_chan, ny) */
    const double *rec_v, *rec_y;                    /* the record's (batch, nv), (batch, ny) */
    double *rec_cost, *rec_price;                   /* the record's (batch), (batch, n_chan) */
    double *total; int *steps;                      /* (batch) each */
};

__global__ void __launch_bounds__(256) k_stage_cost(const StageCostArgs a)
{
    const int C = a.n_chan;
    for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < a.batch; b += (long long)gridDim.x * 256) {
        const double *src = a.lib + a.start[b] + (long long)a.step * C;
        double *price = a.rec_price + b * C;
        for (int c = 0; c < C; ++c) price[c] = src[c];
        const bool usable = a.mask ? a.mask[b] != 0 : (!a.status || plan_usable(a.status, a.obj, (int)b));
        if (!usable) { a.rec_cost[b] = __builtin_nan(""); continue; }      /* skipped: total and steps stay */
        const size_t m = a.model_idx ? a.model_idx[b] : 0;
        const double cost = stage_cost_value(a.w_v + m * C * a.nv, a.w_y + m * C * a.ny, src, a.rec_v + b * a.nv, a.rec_y + b * a.ny, C, a.nv, a.ny);
        a.rec_cost[b] = cost;
        {
            PR_NO_CONTRACT
            a.total[b] = a.total[b] + cost;
        }
        a.steps[b] += 1;
    }
}
#endif
