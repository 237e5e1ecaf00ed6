// Per-instance linear cost (mld_upload_instance_cost): the weights on x_tilde / y_tilde of every instance pulled back through
// the condensed maps (controllers/components/variables.py:259-275; the reference rebuilds its objective per solve() call,
// micro_grid_control_simulation.py:194-198,229) as ONE GEMM per model
//     out[b, :] += [lin_x_b | lin_y_b] [W ; Y],   W = [Gamma_v | Phi_x | Gamma_w | Gamma_5],  Y = [L_v | L_x | L_w | L_5]
// with the instances along M and the n + nx + N nw + 1 output columns along N.  A member of the instance-GEMM family (mfma.inc).
// What it adds: the maps are stored (rows x cols) row-major and the output columns are their columns, so a block of 16 output
// columns is staged as 128-byte row segments into an LDS tile [k][16] (B[k = 4 s + lk][j = li] is then a conflict-free 64-double
// sweep per MFMA); and `out` (pre-loaded with lin_v, or zero) is the accumulator, read and written by the same lane in every chunk.
#pragma once

struct PbMaps {                      // per family [v, x, w, 5]: device pointer (null = zeros) and per-model stride
    const double *W[4], *Y[4];
    size_t sW[4], sY[4];
};

// the column of the stacked maps an output column belongs to: family, column inside it, its row length
__device__ __forceinline__ void pb_column(int c, int n, int nx, int nW, int &fam, int &col, int &ld)
{
    if (c < n) { fam = 0; col = c; ld = n; }
    else if (c < n + nx) { fam = 1; col = c - n; ld = nx; }
    else if (c < n + nx + nW) { fam = 2; col = c - n - nx; ld = nW; }
    else { fam = 3; col = 0; ld = 1; }
}

template <bool F32>
__global__ void __launch_bounds__(64 * RM_WAVES) k_inst_pullback(int NX, int NY, int n, int nx, int nW, PbMaps mp, const RhsGroup *groups,
                                                                 const int *perm, const double *wts, double *out)
{
    __shared__ double pb_tile[IG_KC * 16];
    const RhsGroup g = groups[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int K = NX + NY, ncol = n + nx + nW + 1;
    int oinst[4];
    const int inst = ig_slots<F32>(g, perm, wave, li, lk, oinst);
    for (int kc0 = 0; kc0 < K; kc0 += IG_KC) {
        const int ks = (min(IG_KC, K - kc0) + 3) >> 2;
        IgFrag<F32, IG_KS> a;
        ig_load_a(a, inst, kc0, lk, ks, K, [=](int k) { return wts[(size_t)inst * K + k]; });
        for (int cb = 0; cb < ncol; cb += 16) {
            __syncthreads();
            {   // stage rows kc0 .. kc0 + 4 ks of output columns cb .. cb + 15 (a thread keeps its column: 512 = 0 mod 16)
                const int j = tid & 15, c = cb + j;
                int fam = 0, col = 0, ld = 1;
                pb_column(min(c, ncol - 1), n, nx, nW, fam, col, ld);
                const double *pw = (c < ncol && mp.W[fam]) ? mp.W[fam] + (size_t)g.model * mp.sW[fam] + col : nullptr;
                const double *py = (c < ncol && mp.Y[fam]) ? mp.Y[fam] + (size_t)g.model * mp.sY[fam] + col : nullptr;
                for (int kk = tid >> 4; kk < 4 * ks; kk += (64 * RM_WAVES) >> 4) {
                    const int k = kc0 + kk;
                    double v = 0.0;
                    if (k < NX) { if (pw) v = pw[(size_t)k * ld]; }
                    else if (k < K) { if (py) v = py[(size_t)(k - NX) * ld]; }
                    pb_tile[kk * 16 + j] = v;
                }
            }
            __syncthreads();
            const int c = cb + li;
            double res[4];
            ig_mma<64>(a, pb_tile + lk * 16 + li, IgMask{ig_bits(0, ks)}, res);          // B[k = 4 s + lk][j = li]
            if (c < ncol) {
#pragma unroll
                for (int r = 0; r < 4; ++r) if (oinst[r] >= 0) out[(size_t)oinst[r] * ncol + c] += res[r];
            }
        }
    }
}

// the same on the vector ALUs (MLD_DBG_GEMM_VALU): one workgroup per instance, its weights in LDS, threads own output columns
__global__ void __launch_bounds__(256) k_inst_pullback_valu(int NX, int NY, int n, int nx, int nW, PbMaps mp, const int *model_idx,
                                                            const double *wts, double *out)
{
    extern __shared__ double pb_w[];
    const int b = blockIdx.x, mdl = model_idx ? model_idx[b] : 0;
    const int K = NX + NY, ncol = n + nx + nW + 1;
    for (int k = threadIdx.x; k < K; k += blockDim.x) pb_w[k] = wts[(size_t)b * K + k];
    __syncthreads();
    for (int c = threadIdx.x; c < ncol; c += blockDim.x) {
        int fam, col, ld;
        pb_column(c, n, nx, nW, fam, col, ld);
        double s = 0.0;
        if (mp.W[fam]) { const double *pw = mp.W[fam] + (size_t)mdl * mp.sW[fam] + col; for (int k = 0; k < NX; ++k) s += pb_w[k] * pw[(size_t)k * ld]; }
        if (mp.Y[fam]) { const double *py = mp.Y[fam] + (size_t)mdl * mp.sY[fam] + col; for (int k = 0; k < NY; ++k) s += pb_w[NX + k] * py[(size_t)k * ld]; }
        out[(size_t)b * ncol + c] += s;
    }
}

// At every launch: qs_inst[b, j] = cs[m, j] (q0[m, j] + icost[b, j]) for the dense kernel and, with cs_t, the same under the
// Toeplitz-compatible column scales for the LDS-resident LP (k_lp_lds).  icost: batch x ldi, its first n columns the pulled-back weights.
__global__ void __launch_bounds__(256) k_inst_cost(size_t count, int n, int ldi, const double *q0, const double *cs, const double *cs_t,
                                                  const int *model_idx, const double *icost, double *qs_inst, double *qs_inst_t)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    const size_t b = e / n, j = e - b * n;
    const size_t mj = (size_t)(model_idx ? model_idx[b] : 0) * n + j;
    const double q = q0[mj] + icost[b * ldi + j];
    qs_inst[e] = q * cs[mj];
    if (qs_inst_t) qs_inst_t[e] = q * cs_t[mj];
}

// rconst[b] += cx_b' x0_b + cw_b' omega_b + c0_b with [cx_b | cw_b | c0_b] = columns n .. of icost; a wave per instance
__global__ void __launch_bounds__(256) k_inst_const(int batch, int n, int nx, int nW, int ldi, const double *icost, const double *x0,
                                                   const double *omega, double *rconst)
{
    const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= batch) return;
    const double *c = icost + (size_t)b * ldi + n;
    double acc = 0.0;
    for (int k = lane; k < nx; k += 64) acc += c[k] * x0[(size_t)b * nx + k];
    for (int k = lane; k < nW; k += 64) acc += c[nx + k] * omega[(size_t)b * nW + k];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) rconst[b] += acc + c[nx + nW];
}
