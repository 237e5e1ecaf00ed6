// Predicted trajectories of a resident batch (mld_predict_batch): the state and output variables the reference builds after every solve(),
//     x_tilde = Phi_x x_k + Gamma_v v_tilde + Gamma_omega omega_tilde + Gamma_5      (controllers/components/variables.py:259-265)
//     y_tilde = L_x   x_k + L_v     v_tilde + L_omega     omega_tilde + L_5          (:269-275)
// as ONE GEMM per model, the forward half of k_inst_pullback (inst_cost.inc):
//     [x_tilde_b | y_tilde_b] = [v_b | x0_b | omega_b | 1] . [Gamma_v | Phi_x | Gamma_w | Gamma_5 ; L_v | L_x | L_w | L_5]'
// with the instances along M and the N nx + N ny output rows along N.  A member of the instance-GEMM family (mfma.inc).  What it adds: the
// eight maps read as one stacked matrix with the inner dimension contiguous (row tiles, ig_stage); the causal skip below; the constant column
// (Gamma_5 / L_5 times the trailing 1) added to the first chunk's result as K3 adds H_5, so the multiplied inner dimension is n + nx + N nw
// (cfg4: 782); NaN rows for instances without a usable plan.  The output is the accumulator, written by the first chunk and read and written
// by the same lane in every later one.
//
// Causal skip: block (i, j) of Gamma_v / Gamma_w is zero for j >= i and of L_v / L_w for j > i (the state of step i depends on the inputs of
// the steps before it, the output also on its own step; tests/test_trajectories_host.py pins this on the condensed maps, time-varying
// horizons included).  ONE conservative rule for both families: a 16-row block whose last step is i reads the v and omega columns of steps
// j <= i only.  Groups of four inner indices are staged and multiplied whole, so a group that straddles the boundary reads stored zeros.
#pragma once

// a family's map of this model, or its stride, by number (selects of values, not an indexed array: they stay in registers)
template <typename T> __device__ __forceinline__ T tj_pick(int f, const T (&a)[4])
{
    const T a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    return f == 0 ? a0 : f == 1 ? a1 : f == 2 ? a2 : a3;
}

// status / obj: null = the caller's plans (no masking); else an instance without a usable plan (plan_usable) gets NaN rows
template <bool F32>
__global__ void __launch_bounds__(64 * RM_WAVES) k_trajectory(int N, int nxs, int nys, int nv, int nw, PbMaps mp, const RhsGroup *groups,
                                                              const int *perm, const double *v, const double *x0, const double *omega,
                                                              const int *status, const double *obj, int r_begin, int r_end, double *xo, double *yo)
{
    __shared__ double tj_tile[16 * IG_LD];
    const RhsGroup g = groups[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int NX = N * nxs, NY = N * nys, n = N * nv, nx = nxs, nW = N * nw, K = n + nx + nW;
    int oinst[4]; bool dead[4];
    const int inst = ig_slots<F32>(g, perm, wave, li, lk, oinst);
#pragma unroll
    for (int r = 0; r < 4; ++r) dead[r] = status && oinst[r] >= 0 && !plan_usable(status, obj, oinst[r]);
    for (int kc0 = 0; kc0 < K || kc0 == 0; kc0 += IG_KC) {
        const int ks = (min(IG_KC, K - kc0) + 3) >> 2, g0 = kc0 >> 2;
        IgFrag<F32, IG_KS> a;                   // this chunk of [v | x0 | omega]
        ig_load_a(a, inst, kc0, lk, ks, K, [=](int k) {
            if (k < n) return v[(size_t)inst * n + k];
            if (k < n + nx) return x0[(size_t)inst * nx + (k - n)];
            return omega[(size_t)inst * nW + (k - n - nx)];
        });
        for (int rb = r_begin; rb < r_end; rb += 16) {
            // the last step among the rows of this block, and with it the groups of four inner indices the block needs
            const int last = min(rb + 15, r_end - 1);
            int imax = 0;
            if (rb < NX) imax = min(last, NX - 1) / nxs;
            if (last >= NX) imax = max(imax, (last - NX) / nys);
            // (global groups [0, ga) of v and [n / 4, gc) of x0 and omega; as bits of this chunk)
            const int ga = (min(n, (imax + 1) * nv) + 3) >> 2, gc = (n + nx + min(nW, (imax + 1) * nw) + 3) >> 2;
            const unsigned long long need = (ig_bits(-g0, ga - g0) | ig_bits((n >> 2) - g0, gc - g0)) & ig_bits(0, ks);
            if (!need && kc0 > 0) continue;         // nothing of this chunk reaches these rows (uniform over the workgroup)
            // rows rb .. rb + 15 of the stacked maps, inner indices kc0 .. kc0 + 4 ks
            ig_stage(tj_tile, tid, rb, kc0, need, [=](int row, int k) {
                double val = 0.0;
                if (row < r_end && k < K) {
                    const bool isx = row < NX;
                    const size_t rr = isx ? row : row - NX;
                    int fam, col, ld;
                    pb_column(k, n, nx, nW, fam, col, ld);
                    const double *pm = isx ? tj_pick(fam, mp.W) : tj_pick(fam, mp.Y);
                    const size_t sm = isx ? tj_pick(fam, mp.sW) : tj_pick(fam, mp.sY);
                    if (pm) val = pm[(size_t)g.model * sm + rr * ld + col];
                }
                return val;
            });
            const int row = rb + li;
            double res[4];
            ig_mma<4>(a, tj_tile + li * IG_LD + lk, IgMask{need}, res);      // B = map[rb + li][kc0 + k]
            if (row < r_end) {
                if (kc0 == 0) {      // the constant column
                    const double *p5 = row < NX ? mp.W[3] : mp.Y[3];
                    const double c5 = p5 ? p5[(size_t)g.model * (row < NX ? mp.sW[3] : mp.sY[3]) + (row < NX ? row : row - NX)] : 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) res[r] += c5;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (oinst[r] < 0) continue;
                    double *dst = row < NX ? xo + (size_t)oinst[r] * NX + row : yo + (size_t)oinst[r] * NY + (row - NX);
                    if (dead[r]) *dst = __builtin_nan("");
                    else *dst = kc0 ? *dst + res[r] : res[r];
                }
            }
        }
    }
}

// the same on the vector ALUs (MLD_DBG_GEMM_VALU): one workgroup per instance, its inputs in LDS, a wave per output row with the lanes along
// the inner dimension.  The full product, without the causal skip: agreement with k_trajectory also checks the skip.
__global__ void __launch_bounds__(256) k_trajectory_valu(int NX, int NY, int n, int nx, int nW, PbMaps mp, const int *model_idx, const double *v,
                                                         const double *x0, const double *omega, const int *status, const double *obj,
                                                         int r_begin, int r_end, double *xo, double *yo)
{
    extern __shared__ double tj_in[];
    const int b = blockIdx.x, mdl = model_idx ? model_idx[b] : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int off[4] = {0, n, n + nx, n + nx + nW}, len[4] = {n, nx, nW, 1};
    for (int k = threadIdx.x; k < n; k += blockDim.x) tj_in[k] = v[(size_t)b * n + k];
    for (int k = threadIdx.x; k < nx; k += blockDim.x) tj_in[n + k] = x0[(size_t)b * nx + k];
    for (int k = threadIdx.x; k < nW; k += blockDim.x) tj_in[n + nx + k] = omega[(size_t)b * nW + k];
    if (threadIdx.x == 0) tj_in[n + nx + nW] = 1.0;
    __syncthreads();
    const bool dead = status && !plan_usable(status, obj, b);
    for (int row = r_begin + wave; row < r_end; row += blockDim.x >> 6) {
        const bool isx = row < NX;
        const size_t rr = isx ? row : row - NX;
        double s = 0.0;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const double *base = isx ? mp.W[f] : mp.Y[f];
            if (!base) continue;
            const double *pm = base + (size_t)mdl * (isx ? mp.sW[f] : mp.sY[f]) + rr * len[f];
            for (int k = lane; k < len[f]; k += 64) s += pm[k] * tj_in[off[f] + k];
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) {
            double *dst = isx ? xo + (size_t)b * NX + row : yo + (size_t)b * NY + (row - NX);
            *dst = dead ? __builtin_nan("") : s;
        }
    }
}
