// k_lp_lds: LP relaxations of the condensed MLD problem solved ENTIRELY IN LDS -- the formulation the north star asked for
// ("LDS-staged KKT tiles, coalesced reads of the batched constraint matrices").  Used when every binary of an instance is fixed
// (relaxation-only mode, BASELINE configs[1]: `fixed_bin`), the cost is linear and the model is time invariant.
//
// Revised bounded dual simplex on the working basis (oracle/mld_oracle.c section (4), orc_lp_revised -- same tolerances, same
// Harris ratio test, same Bland fallback).  One workgroup (LP_NT threads) owns an instance.  Resident in LDS for the whole solve:
//   * the COMPACT block-Toeplitz constraint matrix: the N lag blocks of H_v (nc x nv each), pre-scaled with a Toeplitz-compatible
//     equilibration (one factor per row-in-step and per variable-in-step, powers of two): cfg3 25 x 20 x 23 x 8 B = 92 KB.
//     G[(i, c), (j, p)] = blk[i - j][c][p] for j <= i, 0 above the block diagonal;
//   * the explicit inverse of the working basis W = G[T, B] (T tight rows, B basic structurals, k x k, k <= kcap ~ 76);
//   * primal values x (n), s (m), reduced costs d (n), the pivot row alpha (n), basis maps.
// Per pivot: row of W^-1 (or G[i, B] W^-1), the pivot row over all non-basic columns by walking the tight rows' Toeplitz blocks,
// three block reductions for the ratio test, the entering column, O(k^2) update of W^-1 (column replaced / row replaced /
// bordered / row and column deleted).  No dictionary, no HBM traffic inside the loop except q, bounds and h (read-only, L2).
// W^-1 and all values are recomputed from the data every LP_REFRESH pivots and before optimality is declared.
// An instance whose working basis outgrows kcap is reported with status -1 and re-solved by the dense kernel (host side).
#pragma once

#define LP_NT 640                    // 10 waves: the n = 575 columns and m = 500 rows of the cfg3 shape in one sweep
#define LP_NW (LP_NT / 64)
#define LP_REFRESH 100

struct LpShape {
    int n, m, N, nc, nv, kcap, ldw;      // ldw = kcap + 1: odd row stride of W^-1 (column walks without 16-way bank conflicts)
    int nx, nW, max_pivots;
    int f32_off;                         // offset (in doubles) of the fp32 bound arrays inside the dynamic LDS block
};

struct LpModelDev {                      // per model, n_models x ...
    const double *blk;                   // N x nc x nv pre-scaled lag blocks
    const double *qs, *lb, *ub;          // n: scaled cost and bounds
    const double *cs;                    // n: column scales (to un-scale the solution)
    const double *cx, *cw, *c0;          // objective constant r = c0 + cx.x0 + cw.w
    const int *bins; int nb;
    const unsigned char *is_int;         // n (shared by the models): 1 = binary column
};

struct LpBatchDev {
    int batch;
    const int *model_idx;
    const double *x0, *omega, *hs;       // hs: batch x m right-hand sides scaled with the Toeplitz row scales (K3)
    const unsigned char *fixed;          // batch x nb
    double *v_out, *obj_out, *lb_out;
    int *status_out, *nodes_out, *pivots_out;
    long long *ticks_out;
    long long *prof_out;                 // batch x 8 phase ticks (may be null): 0 leaving, 1 rho, 2 pivot row, 3 ratio test, 4 entering column, 5 value updates, 6 W^-1 update, 7 set-up / refresh / verify
    int *counter;
    int *cuts_out;                       // cut rows added (always 0 for an LP; may be null)
    const double *qs_inst, *rconst;      // per-instance linear cost (mld_upload_instance_cost) or null: batch x n scaled like LpModelDev.qs, instead of it; batch, its constant
};

// every member points into LDS and says so: generic pointers would compile to flat_load / flat_store, whose latency is several times
// that of ds_read / ds_write and which tie the LDS and vector-memory counters together (measured: 17 -> us per pivot)
typedef __attribute__((address_space(3))) double lp_f64;
typedef __attribute__((address_space(3))) int lp_i32;
typedef __attribute__((address_space(3))) short lp_i16;
typedef __attribute__((address_space(3))) unsigned char lp_u8;
typedef __attribute__((address_space(3))) float lp_f32;
struct LpLds {
    lp_f64 *blk, *Winv, *x, *s, *d, *alpha, *rho, *w, *dS, *alphaS, *gt;
    lp_i32 *Bs, *T;
    lp_i16 *posB, *posT;
    lp_i16 *Tstep, *Tc, *Bstep, *Bp;     // (step, row-in-step) of the tight rows, (step, variable-in-step) of the basic structurals
    lp_u8 *up, *skipX, *skipS, *fx;      // fx: structural fixed (lo == hi)
    lp_f32 *lo, *hi;                     // bounds of the instance: 0 / 1 / +-S_BIG / +-inf / power-of-two multiples of them -- exact in fp32
};

__device__ __forceinline__ double lp_G(const LpLds &L, const LpShape &S, int row, int col)
{   // G[(i, c), (j, p)] of the compact Toeplitz store
    const int i = row / S.nc, c = row - i * S.nc, j = col / S.nv, p = col - j * S.nv;
    return i >= j ? L.blk[((i - j) * S.nc + c) * S.nv + p] : 0.0;
}

__device__ __forceinline__ void lp_set_T(const LpLds &L, const LpShape &S, int t, int row) { L.T[t] = row; const int i = row / S.nc; L.Tstep[t] = (short)i; L.Tc[t] = (short)(row - i * S.nc); }
__device__ __forceinline__ void lp_set_B(const LpLds &L, const LpShape &S, int p, int col) { L.Bs[p] = col; const int j = col / S.nv; L.Bstep[p] = (short)j; L.Bp[p] = (short)(col - j * S.nv); }

struct LpShared { double rv[2][LP_NW]; int ri[2][LP_NW]; int rj[2][LP_NW]; };

// block reductions with ONE barrier each: the waves' partial results go to one of two alternating buffers; a wave can only reach the
// reduction after the next one (same buffer) once every wave has passed the barrier in between, i.e. has finished reading.
__device__ __forceinline__ double lp_block_max(LpShared &sh, double v, int &par)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    par ^= 1;
    if ((threadIdx.x & 63) == 0) sh.rv[par][threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh.rv[par][0];
#pragma unroll
    for (int q = 1; q < LP_NW; ++q) s = fmax(s, sh.rv[par][q]);
    return s;
}
__device__ __forceinline__ double lp_block_min(LpShared &sh, double v, int &par) { return -lp_block_max(sh, -v, par); }
__device__ __forceinline__ double lp_block_sum(LpShared &sh, double v, int &par)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    par ^= 1;
    if ((threadIdx.x & 63) == 0) sh.rv[par][threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < LP_NW; ++q) s += sh.rv[par][q];
    return s;
}
// arg-max with smallest-index tie break (index -1 = none)
__device__ __forceinline__ int lp_block_argmax(LpShared &sh, double v, int idx, double *out, int &par)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_down(v, o, 64); const int i2 = __shfl_down(idx, o, 64);
        if (v2 > v || (v2 == v && i2 >= 0 && (idx < 0 || i2 < idx))) { v = v2; idx = i2; }
    }
    par ^= 1;
    if ((threadIdx.x & 63) == 0) { sh.rv[par][threadIdx.x >> 6] = v; sh.ri[par][threadIdx.x >> 6] = idx; }
    __syncthreads();
    double bv = sh.rv[par][0]; int bi = sh.ri[par][0];
#pragma unroll
    for (int q = 1; q < LP_NW; ++q) { const double v2 = sh.rv[par][q]; const int i2 = sh.ri[par][q]; if (v2 > bv || (v2 == bv && i2 >= 0 && (bi < 0 || i2 < bi))) { bv = v2; bi = i2; } }
    *out = bv;
    return bi;
}
__device__ __forceinline__ int lp_block_argmin_int(LpShared &sh, int key, int payload, int &par)
{
    for (int o = 32; o > 0; o >>= 1) { const int k2 = __shfl_down(key, o, 64), p2 = __shfl_down(payload, o, 64); if (k2 < key) { key = k2; payload = p2; } }
    par ^= 1;
    if ((threadIdx.x & 63) == 0) { sh.ri[par][threadIdx.x >> 6] = key; sh.rj[par][threadIdx.x >> 6] = payload; }
    __syncthreads();
    int bk = sh.ri[par][0], bp = sh.rj[par][0];
#pragma unroll
    for (int q = 1; q < LP_NW; ++q) if (sh.ri[par][q] < bk) { bk = sh.ri[par][q]; bp = sh.rj[par][q]; }
    return bk == 0x7fffffff ? -1 : bp;
}

// W^-1 (in place, Gauss-Jordan with partial pivoting) and every primal / dual value from the data.  Returns false when W is singular.
__device__ bool lp_refresh(const LpLds &L, const LpShape &S, LpShared &sh, int &par, int k, const double *h, const double *q)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ldw = S.ldw, n = S.n, m = S.m;
    __syncthreads();
    // W[t][p] = G[T_t, B_p], stored at Winv[t * ldw + p]; inverted in place: afterwards Winv[p * ldw + t] = (W^-1)[p][t]
    for (int e = tid; e < k * k; e += LP_NT) { const int t = e / k, p = e - t * k; L.Winv[t * ldw + p] = lp_G(L, S, L.T[t], L.Bs[p]); }
    __syncthreads();
    lp_i16 *perm = (lp_i16 *)L.alphaS;       // k row swaps (alphaS is free here: kcap doubles >= k shorts)
    for (int c = 0; c < k; ++c) {
        double mv = -1.0; int mi = -1;
        for (int a = c + tid; a < k; a += LP_NT) { const double v = fabs(L.Winv[a * ldw + c]); if (v > mv) { mv = v; mi = a; } }
        double bv;
        const int pv = lp_block_argmax(sh, mv, mi, &bv, par);
        if (pv < 0 || !(bv > 1e-13)) return false;
        if (tid == 0) perm[c] = (short)pv;
        if (pv != c) for (int b = tid; b < k; b += LP_NT) { const double t2 = L.Winv[c * ldw + b]; L.Winv[c * ldw + b] = L.Winv[pv * ldw + b]; L.Winv[pv * ldw + b] = t2; }
        __syncthreads();
        const double piv = L.Winv[c * ldw + c];
        __syncthreads();
        const double inv = 1.0 / piv;
        for (int b = tid; b < k; b += LP_NT) L.Winv[c * ldw + b] = (b == c) ? inv : L.Winv[c * ldw + b] * inv;
        for (int a = tid; a < k; a += LP_NT) L.gt[a] = (a == c) ? 0.0 : L.Winv[a * ldw + c];       // multipliers (column c before it is overwritten)
        __syncthreads();
        for (int a = wave; a < k; a += LP_NW) {
            const double f = L.gt[a];
            if (a == c || f == 0.0) continue;
            for (int b = lane; b < k; b += 64) L.Winv[a * ldw + b] = (b == c ? 0.0 : L.Winv[a * ldw + b]) - f * L.Winv[c * ldw + b];
        }
        __syncthreads();
    }
    for (int c = k - 1; c >= 0; --c) {       // undo the row swaps as column swaps, in reverse order
        const int pv = perm[c];
        if (pv != c) for (int a = tid; a < k; a += LP_NT) { const double t2 = L.Winv[a * ldw + c]; L.Winv[a * ldw + c] = L.Winv[a * ldw + pv]; L.Winv[a * ldw + pv] = t2; }
        __syncthreads();
    }
    // x_B = W^-1 (h_T - G[T, N] x_N): a wave per tight row for the right-hand side (gt), then a wave per basic structural
    for (int t = wave; t < k; t += LP_NW) {
        const int row = L.T[t], i = row / S.nc, c = row - i * S.nc, jmax = (i + 1) * S.nv;
        double a = 0.0;
        for (int j = lane; j < jmax; j += 64) if (L.posB[j] < 0) { const int jj = j / S.nv, p = j - jj * S.nv; a += L.blk[((i - jj) * S.nc + c) * S.nv + p] * L.x[j]; }
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
        if (lane == 0) L.gt[t] = h[row] - a;
    }
    __syncthreads();
    for (int p = wave; p < k; p += LP_NW) {
        double a = 0.0;
        for (int t = lane; t < k; t += 64) a += L.Winv[p * ldw + t] * L.gt[t];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
        if (lane == 0) L.x[L.Bs[p]] = a;
    }
    __syncthreads();
    for (int row = tid; row < m; row += LP_NT) {        // a thread per row: x[j] is a broadcast read, the row's blocks are walked lag by lag
        if (L.posT[row] >= 0) { L.s[row] = 0.0; continue; }
        const int i = row / S.nc, c = row - i * S.nc;
        double a = 0.0;
        for (int jj = 0; jj <= i; ++jj) {
            const lp_f64 *b = L.blk + ((i - jj) * S.nc + c) * S.nv;
            const lp_f64 *xx = L.x + jj * S.nv;
            for (int p = 0; p < S.nv; ++p) a += b[p] * xx[p];
        }
        L.s[row] = h[row] - a;
    }
    // pi = W^-T q_B (into gt), d_j = q_j - pi . G[T, j], dS_t = -pi_t
    __syncthreads();
    for (int p = tid; p < k; p += LP_NT) L.w[p] = q[L.Bs[p]];
    __syncthreads();
    for (int t = tid; t < k; t += LP_NT) { double a = 0.0; for (int p = 0; p < k; ++p) a += L.Winv[p * ldw + t] * L.w[p]; L.gt[t] = a; L.dS[t] = -a; }
    __syncthreads();
    for (int j = tid; j < n; j += LP_NT) {
        if (L.posB[j] >= 0) { L.d[j] = 0.0; continue; }
        const int jj = j / S.nv, p = j - jj * S.nv;
        double a = q[j];
        for (int t = 0; t < k; ++t) { const int i = L.Tstep[t]; if (i >= jj) a -= L.gt[t] * L.blk[((i - jj) * S.nc + L.Tc[t]) * S.nv + p]; }
        L.d[j] = a;
    }
    __syncthreads();
    return true;
}

// Verification of an optimum without re-inverting W: the slacks recomputed from x and the data (tight rows must be at zero, the others
// non-negative, basic structurals inside their bounds), and the duals by one step of iterative refinement -- pi = W^-T q_B, residual
// q_B - W' pi against the exact W -- before the reduced costs are recomputed from pi and their signs checked.  Returns the largest
// violation found (primal or dual); the caller falls back to lp_refresh() when it is not negligible.
__device__ double lp_verify(const LpLds &L, const LpShape &S, LpShared &sh, int &par, int k, const double *h, const double *q, const lp_f32 *lo, const lp_f32 *hi)
{
    const int tid = threadIdx.x, ldw = S.ldw, n = S.n, m = S.m;
    double worst = 0.0;
    __syncthreads();
    for (int row = tid; row < m; row += LP_NT) {
        const int i = row / S.nc, c = row - i * S.nc;
        double a = 0.0;
        for (int jj = 0; jj <= i; ++jj) {
            const lp_f64 *b = L.blk + ((i - jj) * S.nc + c) * S.nv;
            const lp_f64 *xx = L.x + jj * S.nv;
            for (int p = 0; p < S.nv; ++p) a += b[p] * xx[p];
        }
        const double sv = h[row] - a;
        worst = fmax(worst, L.posT[row] >= 0 ? fabs(sv) : (L.skipS[row] ? 0.0 : -sv));
    }
    for (int p = tid; p < k; p += LP_NT) { const int j = L.Bs[p]; if (!L.skipX[j]) worst = fmax(worst, fmax((double)lo[j] - L.x[j], L.x[j] - (double)hi[j])); L.w[p] = q[j]; }
    __syncthreads();
    for (int t = tid; t < k; t += LP_NT) { double a = 0.0; for (int p = 0; p < k; ++p) a += L.Winv[p * ldw + t] * L.w[p]; L.gt[t] = a; }
    __syncthreads();
    for (int p = tid; p < k; p += LP_NT) {      // residual of W' pi = q_B for basic structural p: q_p - sum_t G[T_t, B_p] pi_t
        const int jj = L.Bstep[p], pp = L.Bp[p];
        double a = L.w[p];
        for (int t = 0; t < k; ++t) { const int i = L.Tstep[t]; if (i >= jj) a -= L.gt[t] * L.blk[((i - jj) * S.nc + L.Tc[t]) * S.nv + pp]; }
        worst = fmax(worst, fabs(a));
    }
    for (int t = tid; t < k; t += LP_NT) worst = fmax(worst, L.gt[t]);        // slack reduced cost -pi_t must be >= 0
    for (int j = tid; j < n; j += LP_NT) {
        if (L.posB[j] >= 0 || L.fx[j]) continue;
        const int jj = j / S.nv, p = j - jj * S.nv;
        double a = q[j];
        for (int t = 0; t < k; ++t) { const int i = L.Tstep[t]; if (i >= jj) a -= L.gt[t] * L.blk[((i - jj) * S.nc + L.Tc[t]) * S.nv + p]; }
        worst = fmax(worst, L.up[j] ? a : -a);
    }
    return lp_block_max(sh, worst, par);
}

__global__ void __launch_bounds__(LP_NT) k_lp_lds(LpShape S, LpModelDev M, LpBatchDev B, unsigned char *ws_base)
{
    extern __shared__ double lp_lds[];
    __shared__ LpShared sh;
    __shared__ int s_inst;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S.n, m = S.m, kc = S.kcap, ldw = S.ldw;
    LpLds L;
    {
        lp_f64 *o = (lp_f64 *)lp_lds;
        L.blk = o; o += S.N * S.nc * S.nv;
        L.Winv = o; o += kc * ldw;
        L.x = o; o += n; L.s = o; o += m; L.d = o; o += n; L.alpha = o; o += n;
        L.rho = o; o += kc; L.w = o; o += kc; L.dS = o; o += kc; L.alphaS = o; o += kc; L.gt = o; o += kc;
        L.Bs = (lp_i32 *)o; L.T = L.Bs + kc; o += kc;        // 2 x kcap ints = kcap doubles
        L.posB = (lp_i16 *)o; L.posT = L.posB + n; L.Tstep = L.posT + m; L.Tc = L.Tstep + kc; L.Bstep = L.Tc + kc; L.Bp = L.Bstep + kc;
        lp_u8 *u8 = (lp_u8 *)(L.Bp + kc);
        L.up = u8; L.skipX = u8 + n; L.skipS = u8 + 2 * n; L.fx = u8 + 2 * n + m;
        L.lo = (lp_f32 *)((lp_f64 *)lp_lds + S.f32_off); L.hi = L.lo + n;
    }
    lp_f32 *lo = L.lo, *hi = L.hi;
    (void)ws_base;
    int cur_model = -1, par = 0;
    __shared__ long long prof[8];
    long long tph = 0;
#define LP_TICK(slot) do { if (tid == 0) { const long long now_ = wall_clock64(); prof[slot] += now_ - tph; tph = now_; } } while (0)
    for (;;) {
        __syncthreads();
        if (tid == 0) s_inst = atomicAdd(B.counter, 1);
        __syncthreads();
        if (s_inst >= B.batch) break;
        const int inst = s_inst, mdl = B.model_idx ? B.model_idx[inst] : 0;
        const long long t_begin = wall_clock64();
        if (tid == 0) { for (int u = 0; u < 8; ++u) prof[u] = 0; tph = t_begin; }
        if (mdl != cur_model) {      // the model's Toeplitz blocks stay in LDS across its instances
            const double *g = M.blk + (size_t)mdl * S.N * S.nc * S.nv;
            for (int e = tid; e < S.N * S.nc * S.nv; e += LP_NT) L.blk[e] = g[e];
            cur_model = mdl;
        }
        const double *q = B.qs_inst ? B.qs_inst + (size_t)inst * n : M.qs + (size_t)mdl * n, *plb = M.lb + (size_t)mdl * n, *pub = M.ub + (size_t)mdl * n;
        const double *h = B.hs + (size_t)inst * m;
        const unsigned char *fixed = B.fixed ? B.fixed + (size_t)inst * M.nb : nullptr;
        // ---- slack basis: every structural non-basic at its dual-feasible bound (free variables boxed only where they must rest)
        for (int j = tid; j < n; j += LP_NT) { lo[j] = (float)plb[j]; hi[j] = (float)pub[j]; }
        __syncthreads();
        if (fixed) for (int kb = tid; kb < M.nb; kb += LP_NT) if (fixed[kb] != 255) { const int j = M.bins[kb]; lo[j] = hi[j] = (float)fixed[kb]; }
        __syncthreads();
        for (int j = tid; j < n; j += LP_NT) {
            const double qj = q[j];
            double l = lo[j], u = hi[j];
            L.posB[j] = -1; L.skipX[j] = 0; L.fx[j] = l == u;
            if (l == u) { L.up[j] = 0; L.x[j] = l; }
            else if (qj >= 0) { if (l == -S_INF) { l = -S_BIG; lo[j] = (float)l; } L.up[j] = 0; L.x[j] = l; }
            else { if (u == S_INF) { u = S_BIG; hi[j] = (float)u; } L.up[j] = 1; L.x[j] = u; }
        }
        for (int i = tid; i < m; i += LP_NT) { L.posT[i] = -1; L.skipS[i] = 0; }
        __syncthreads();
        int k = 0, status = MLD_STATUS_NUMERICAL, pivots = 0, since = 0, stall = 0;
        double last_obj = -S_INF, cur = 0.0;     // dual objective relative to the start: grows by theta * d_q per pivot
        lp_refresh(L, S, sh, par, 0, h, q);
        LP_TICK(7);
        for (;;) {
            __syncthreads();
            if (pivots >= S.max_pivots) { status = MLD_STATUS_NUMERICAL; break; }
            if (since >= LP_REFRESH) { since = 0; if (!lp_refresh(L, S, sh, par, k, h, q)) { status = MLD_STATUS_NUMERICAL; break; } LP_TICK(7); }
            if (cur > last_obj + 1e-12 * fmax(1.0, fabs(cur))) { stall = 0; last_obj = cur; } else stall++;
            const bool bland = stall > 30;
            // ---- leaving variable: largest bound violation (smallest id while stalling); ids: structural j, slack n + i
            double mv = S_PTOL; int mi = -1, bid = 0x7fffffff;
            for (int p = tid; p < k; p += LP_NT) {
                const int j = L.Bs[p];
                if (L.skipX[j]) continue;
                const double v = fmax((double)lo[j] - L.x[j], L.x[j] - (double)hi[j]);
                if (v > S_PTOL) { if (v > mv || (v == mv && (mi < 0 || j < mi))) { mv = v; mi = j; } if (j < bid) bid = j; }
            }
            for (int i = tid; i < m; i += LP_NT) {
                if (L.posT[i] >= 0 || L.skipS[i]) continue;
                const double v = -L.s[i];
                if (v > S_PTOL) { if (v > mv || (v == mv && (mi < 0 || n + i < mi))) { mv = v; mi = n + i; } if (n + i < bid) bid = n + i; }
            }
            double bv;
            int lv = lp_block_argmax(sh, mi >= 0 ? mv : -S_INF, mi, &bv, par);
            LP_TICK(0);
            if (lv < 0) {
                if (since > 0) {
                    since = 0;
                    if (lp_verify(L, S, sh, par, k, h, q, lo, hi) <= 1e-7) { LP_TICK(7); status = MLD_STATUS_OPTIMAL; break; }
                    if (!lp_refresh(L, S, sh, par, k, h, q)) { status = MLD_STATUS_NUMERICAL; break; }
                    continue;
                }
                status = MLD_STATUS_OPTIMAL; break;
            }
            if (bland) lv = lp_block_argmin_int(sh, bid, bid, par);
            // ---- its dictionary row: rho, then alpha over the non-basic structurals and alphaS over the tight rows' slacks
            bool below; double viol, xl;
            if (lv < n) {
                const int p = L.posB[lv];
                for (int t = tid; t < k; t += LP_NT) { const double r0 = L.Winv[p * ldw + t]; L.rho[t] = r0; L.alphaS[t] = r0; }
                xl = L.x[lv];
                const double vlo = (double)lo[lv] - xl, vhi = xl - (double)hi[lv];
                below = vlo > vhi; viol = below ? vlo : vhi;
            } else {
                const int row = lv - n;
                for (int p = tid; p < k; p += LP_NT) L.gt[p] = lp_G(L, S, row, L.Bs[p]);
                __syncthreads();
                for (int t = tid; t < k; t += LP_NT) { double a = 0.0; for (int p = 0; p < k; ++p) a += L.gt[p] * L.Winv[p * ldw + t]; L.rho[t] = a; L.alphaS[t] = -a; }
                xl = L.s[row]; below = true; viol = -xl;
            }
            __syncthreads();
            LP_TICK(1);
            {
                const int lrow = lv >= n ? lv - n : -1, li = lrow >= 0 ? lrow / S.nc : 0, lc = lrow >= 0 ? lrow - li * S.nc : 0;
                for (int j = tid; j < n; j += LP_NT) {
                    if (L.posB[j] >= 0) { L.alpha[j] = 0.0; continue; }
                    const int jj = j / S.nv, p = j - jj * S.nv;
                    double a = 0.0;
                    for (int t = 0; t < k; ++t) {
                        const double r0 = L.rho[t];
                        const int i = L.Tstep[t];
                        if (r0 != 0.0 && i >= jj) a += r0 * L.blk[((i - jj) * S.nc + L.Tc[t]) * S.nv + p];
                    }
                    L.alpha[j] = lrow >= 0 ? ((li >= jj ? L.blk[((li - jj) * S.nc + lc) * S.nv + p] : 0.0) - a) : a;
                }
            }
            __syncthreads();
            LP_TICK(2);
            // ---- ratio test (Harris two-pass)
            double emax = 0.0;
            for (int j = tid; j < n; j += LP_NT) {
                if (L.posB[j] >= 0 || L.fx[j]) continue;
                const double a = L.alpha[j];
                const bool el = below ? (L.up[j] ? a > 0 : a < 0) : (L.up[j] ? a < 0 : a > 0);
                if (el) emax = fmax(emax, fabs(a));
            }
            for (int t = tid; t < k; t += LP_NT) { const double a = L.alphaS[t]; if (below ? a < 0 : a > 0) emax = fmax(emax, fabs(a)); }
            emax = lp_block_max(sh, emax, par);
            const double ptol = fmax(S_PIV_ABS, S_PIV_REL * emax);
            double tmax = S_INF, rmin = S_INF;
            for (int j = tid; j < n; j += LP_NT) {
                if (L.posB[j] >= 0 || L.fx[j]) continue;
                const double a = L.alpha[j];
                const bool el = below ? (L.up[j] ? a > 0 : a < 0) : (L.up[j] ? a < 0 : a > 0);
                if (!el || fabs(a) <= ptol) continue;
                const double da = fmax(L.up[j] ? -L.d[j] : L.d[j], 0.0);
                tmax = fmin(tmax, (da + S_DTOL) / fabs(a)); rmin = fmin(rmin, da / fabs(a));
            }
            for (int t = tid; t < k; t += LP_NT) {
                const double a = L.alphaS[t];
                if (!(below ? a < 0 : a > 0) || fabs(a) <= ptol) continue;
                const double da = fmax(L.dS[t], 0.0);
                tmax = fmin(tmax, (da + S_DTOL) / fabs(a)); rmin = fmin(rmin, da / fabs(a));
            }
            tmax = lp_block_min(sh, tmax, par);
            if (tmax == S_INF) {
                if (viol <= S_PTOL_SKIP) { __syncthreads(); if (tid == 0) { if (lv < n) L.skipX[lv] = 1; else L.skipS[lv - n] = 1; } continue; }
                if (since > 0) { since = 0; if (!lp_refresh(L, S, sh, par, k, h, q)) { status = MLD_STATUS_NUMERICAL; break; } continue; }
                status = MLD_STATUS_INFEASIBLE; break;
            }
            int qent;        // structural j, or n + position t of a tight row's slack
            if (bland) {
                rmin = lp_block_min(sh, rmin, par);
                int key = 0x7fffffff, pay = -1;
                for (int j = tid; j < n; j += LP_NT) {
                    if (L.posB[j] >= 0 || L.fx[j]) continue;
                    const double a = L.alpha[j];
                    const bool el = below ? (L.up[j] ? a > 0 : a < 0) : (L.up[j] ? a < 0 : a > 0);
                    if (!el || fabs(a) <= ptol) continue;
                    if (fmax(L.up[j] ? -L.d[j] : L.d[j], 0.0) / fabs(a) <= rmin * (1 + 1e-12) + 1e-300 && j < key) { key = j; pay = j; }
                }
                for (int t = tid; t < k; t += LP_NT) {
                    const double a = L.alphaS[t];
                    if (!(below ? a < 0 : a > 0) || fabs(a) <= ptol) continue;
                    if (fmax(L.dS[t], 0.0) / fabs(a) <= rmin * (1 + 1e-12) + 1e-300 && n + L.T[t] < key) { key = n + L.T[t]; pay = n + t; }
                }
                qent = lp_block_argmin_int(sh, key, pay, par);
            } else {
                double av = -1.0; int ai = -1;
                for (int j = tid; j < n; j += LP_NT) {
                    if (L.posB[j] >= 0 || L.fx[j]) continue;
                    const double a = L.alpha[j];
                    const bool el = below ? (L.up[j] ? a > 0 : a < 0) : (L.up[j] ? a < 0 : a > 0);
                    if (!el || fabs(a) <= ptol) continue;
                    if (fmax(L.up[j] ? -L.d[j] : L.d[j], 0.0) / fabs(a) <= tmax && fabs(a) > av) { av = fabs(a); ai = j; }
                }
                for (int t = tid; t < k; t += LP_NT) {
                    const double a = L.alphaS[t];
                    if (!(below ? a < 0 : a > 0) || fabs(a) <= ptol) continue;
                    if (fmax(L.dS[t], 0.0) / fabs(a) <= tmax && fabs(a) > av) { av = fabs(a); ai = n + t; }
                }
                double tmp;
                qent = lp_block_argmax(sh, av, ai, &tmp, par);
            }
            LP_TICK(3);
            if (qent < 0) { status = MLD_STATUS_INFEASIBLE; break; }
            const double aq = qent < n ? L.alpha[qent] : L.alphaS[qent - n];
            if (fabs(aq) < S_PIV_TINY && viol <= S_PTOL_SKIP) { __syncthreads(); if (tid == 0) { if (lv < n) L.skipX[lv] = 1; else L.skipS[lv - n] = 1; } continue; }
            if (qent < n && lv >= n && k + 1 > kc) { status = -1; break; }          // working basis outgrows LDS: the dense kernel takes the instance
            // ---- entering column: w over the basic structurals (a wave per entry), then the basic slacks
            if (qent < n) {
                for (int t = tid; t < k; t += LP_NT) L.gt[t] = lp_G(L, S, L.T[t], qent);
                __syncthreads();
                for (int p = wave; p < k; p += LP_NW) {
                    double a = 0.0;
                    for (int t = lane; t < k; t += 64) a += L.Winv[p * ldw + t] * L.gt[t];
                    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
                    if (lane == 0) L.w[p] = a;
                }
            } else for (int p = tid; p < k; p += LP_NT) L.w[p] = L.Winv[p * ldw + (qent - n)];
            __syncthreads();
            const double leave_value = lv < n ? (double)(below ? lo[lv] : hi[lv]) : 0.0;
            const double theta = (xl - leave_value) / aq;
            const double dq = qent < n ? L.d[qent] : L.dS[qent - n];
            const double tau = dq / aq;
            __syncthreads();
            LP_TICK(4);
            for (int p = tid; p < k; p += LP_NT) L.x[L.Bs[p]] -= L.w[p] * theta;
            {
                const int qj = qent < n ? qent / S.nv : 0, qp = qent < n ? qent - qj * S.nv : 0;
                for (int i = tid; i < m; i += LP_NT) {
                    if (L.posT[i] >= 0) continue;
                    const int si = i / S.nc, sc = i - si * S.nc;
                    double c = (qent < n && si >= qj) ? L.blk[((si - qj) * S.nc + sc) * S.nv + qp] : 0.0;
                    for (int p = 0; p < k; ++p) {
                        const double wp = L.w[p];
                        const int jj = L.Bstep[p];
                        if (wp != 0.0 && si >= jj) c -= L.blk[((si - jj) * S.nc + sc) * S.nv + L.Bp[p]] * wp;
                    }
                    L.s[i] -= c * theta;
                }
            }
            for (int j = tid; j < n; j += LP_NT) if (L.posB[j] < 0) L.d[j] -= tau * L.alpha[j];
            for (int t = tid; t < k; t += LP_NT) L.dS[t] -= tau * L.alphaS[t];
            __syncthreads();
            LP_TICK(5);
            // ---- basis change: O(k^2) update of W^-1
            if (qent < n && lv < n) {                        // column p of W replaced
                const int p = L.posB[lv];
                const double inv = 1.0 / L.w[p];
                for (int t = tid; t < k; t += LP_NT) L.Winv[p * ldw + t] *= inv;
                __syncthreads();
                for (int a = wave; a < k; a += LP_NW) { const double f = L.w[a]; if (a != p && f != 0.0) for (int t = lane; t < k; t += 64) L.Winv[a * ldw + t] -= f * L.Winv[p * ldw + t]; }
                __syncthreads();
                if (tid == 0) {
                    L.x[qent] += theta; L.x[lv] = leave_value;
                    lp_set_B(L, S, p, qent); L.posB[qent] = (short)p; L.posB[lv] = -1;
                    L.up[lv] = (leave_value == (double)hi[lv]) && (lo[lv] != hi[lv]);
                    L.d[lv] = -tau; L.d[qent] = 0.0;
                }
            } else if (qent >= n && lv >= n) {               // row t of W replaced
                const int t = qent - n, i = lv - n, told = L.T[t];
                const double inv = 1.0 / L.rho[t];
                for (int p = tid; p < k; p += LP_NT) L.Winv[p * ldw + t] *= inv;
                __syncthreads();
                for (int p = wave; p < k; p += LP_NW) { const double ct = L.Winv[p * ldw + t]; for (int b = lane; b < k; b += 64) if (b != t) L.Winv[p * ldw + b] -= L.rho[b] * ct; }
                __syncthreads();
                if (tid == 0) { L.s[told] = theta; L.s[i] = 0.0; lp_set_T(L, S, t, i); L.posT[i] = (short)t; L.posT[told] = -1; L.dS[t] = -tau; }
            } else if (qent < n && lv >= n) {                // W bordered by row i and column q
                const int i = lv - n;
                const double inv = 1.0 / aq;
                for (int p = wave; p < k; p += LP_NW) { const double f = L.w[p] * inv; for (int t = lane; t < k; t += 64) L.Winv[p * ldw + t] += f * L.rho[t]; }
                for (int p = tid; p < k; p += LP_NT) L.Winv[p * ldw + k] = -L.w[p] * inv;
                for (int t = tid; t < k; t += LP_NT) L.Winv[k * ldw + t] = -L.rho[t] * inv;
                __syncthreads();
                if (tid == 0) {
                    L.Winv[k * ldw + k] = inv;
                    L.x[qent] += theta; L.s[i] = 0.0;
                    lp_set_B(L, S, k, qent); L.posB[qent] = (short)k; lp_set_T(L, S, k, i); L.posT[i] = (short)k;
                    L.dS[k] = -tau; L.d[qent] = 0.0;
                }
                k++;
            } else {                                         // row t and column p of W removed
                const int t = qent - n, p = L.posB[lv], told = L.T[t], last = k - 1;
                const double inv = 1.0 / L.Winv[p * ldw + t];
                for (int a = tid; a < k; a += LP_NT) L.gt[a] = L.Winv[a * ldw + t] * inv;
                __syncthreads();
                for (int a = wave; a < k; a += LP_NW) { const double f = L.gt[a]; if (a != p && f != 0.0) for (int b = lane; b < k; b += 64) if (b != t) L.Winv[a * ldw + b] -= f * L.Winv[p * ldw + b]; }
                __syncthreads();
                // compact: the last position moves into the holes (row p <- last row, column t <- last column)
                if (p != last) for (int b = tid; b < k; b += LP_NT) L.Winv[p * ldw + b] = L.Winv[last * ldw + b];
                __syncthreads();
                if (t != last) for (int a = tid; a < k; a += LP_NT) L.Winv[a * ldw + t] = L.Winv[a * ldw + last];
                __syncthreads();
                if (tid == 0) {
                    L.s[told] = theta; L.x[lv] = leave_value;
                    L.posB[lv] = -1; L.posT[told] = -1;
                    L.up[lv] = (leave_value == (double)hi[lv]) && (lo[lv] != hi[lv]);
                    L.d[lv] = -tau;
                    if (p != last) { lp_set_B(L, S, p, L.Bs[last]); L.posB[L.Bs[p]] = (short)p; }
                    if (t != last) { lp_set_T(L, S, t, L.T[last]); L.posT[L.T[t]] = (short)t; L.dS[t] = L.dS[last]; }
                }
                k--;
            }
            cur += theta * dq;
            pivots++; since++;
            LP_TICK(6);
        }
        // ---- results
        __syncthreads();
        double *v_out = B.v_out + (size_t)inst * n;
        if (status == MLD_STATUS_OPTIMAL) {
            // a free variable resting non-basic on the artificial box with a non-zero reduced cost: the objective falls along its ray
            double hit = 0.0;
            for (int j = tid; j < n; j += LP_NT) {
                if (L.posB[j] >= 0 || fabs(L.d[j]) <= 1e-9) continue;
                if ((plb[j] == -S_INF && L.x[j] <= -0.999 * S_BIG) || (pub[j] == S_INF && L.x[j] >= 0.999 * S_BIG)) hit = 1.0;
            }
            if (lp_block_max(sh, hit, par) > 0.0) status = MLD_STATUS_UNBOUNDED;
        }
        if (status == MLD_STATUS_UNBOUNDED) {
            const double *cs = M.cs + (size_t)mdl * n;
            for (int j = tid; j < n; j += LP_NT) v_out[j] = L.x[j] * cs[j];
            if (tid == 0) { B.obj_out[inst] = -S_INF; B.lb_out[inst] = -S_INF; }
        } else if (status == MLD_STATUS_OPTIMAL) {
            const double *cs = M.cs + (size_t)mdl * n;
            double part = 0.0;
            for (int j = tid; j < n; j += LP_NT) { v_out[j] = L.x[j] * cs[j]; part += q[j] * L.x[j]; }
            const double ob = lp_block_sum(sh, part, par);
            if (tid == 0) {
                double r = 0.0;
                if (M.c0) r += M.c0[mdl];
                if (M.cx) for (int j = 0; j < S.nx; ++j) r += M.cx[(size_t)mdl * S.nx + j] * B.x0[(size_t)inst * S.nx + j];
                if (M.cw) for (int j = 0; j < S.nW; ++j) r += M.cw[(size_t)mdl * S.nW + j] * B.omega[(size_t)inst * S.nW + j];
                if (B.rconst) r += B.rconst[inst];
                B.obj_out[inst] = ob + r; B.lb_out[inst] = ob + r;
            }
        } else {
            for (int j = tid; j < n; j += LP_NT) v_out[j] = 0.0;
            if (tid == 0) { B.obj_out[inst] = S_INF; B.lb_out[inst] = -S_INF; }
        }
        if (tid == 0) { B.status_out[inst] = status; B.nodes_out[inst] = 1; B.pivots_out[inst] = pivots; B.ticks_out[inst] = wall_clock64() - t_begin;
                        if (B.prof_out) for (int u = 0; u < 8; ++u) B.prof_out[(size_t)inst * 8 + u] = prof[u]; }
    }
}
