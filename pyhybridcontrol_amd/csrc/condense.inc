// Kernels K1 + K2: condensing an MLD model over the horizon, on device, for n_models models at once.
//
// Replaces controllers/components/mld_evolution_matrices.py:137-244,253-332,467-527 and the
// block_toeplitz / block_diag_dense assembly of utils/matrix_utils.py:55-81,117-161.
//
// Design (MI355X): the reference multiplies (N nc x N nx) block-diagonal matrices with (N nx x N nv)
// block-Toeplitz ones -- O(N^3) flops of which all but O(N) are multiplications by structural zeros.
// Here only the N distinct blocks per family are computed (k_condense_blocks, one workgroup per model,
// a few hundred KB that stay in L2), then k_condense_flat streams them into the reference's exact
// materialised layout.  The scatter is a pure HBM write stream: every output matrix is one flat array,
// a workgroup owns a 16-byte aligned chunk of it and every wave-instruction stores 1 KiB contiguously
// (k_condense_scatter, one workgroup per block of rows, remains as the fallback for > 2^32 elements).  Algorithmic bytes
// per model = sum of the 12 output sizes + the 20 inputs (SURVEY 8d); flops are negligible
// (K = nx <= 15 in every BASELINE config), so the matrix cores have nothing to do here.
#pragma once
#include "common.h"

void compute_layout(const mld_dims &d, int N, CondLayout *L)
{
    L->nx = d.nx; L->nu = d.nu; L->nd = d.ndelta; L->nz = d.nz; L->nmu = d.nmu; L->nw = d.nomega;
    L->ny = d.ny; L->nc = d.nc; L->nv = d.nu + d.ndelta + d.nz + d.nmu; L->N = N;
    L->rows[0] = d.nx; L->rows[1] = d.ny; L->rows[2] = d.nc;
    size_t o = 0;
    for (int f = 0; f < 3; ++f) { L->offV[f] = o; o += (size_t)N * L->rows[f] * L->nv; }
    for (int f = 0; f < 3; ++f) { L->offW[f] = o; o += (size_t)N * L->rows[f] * L->nw; }
    for (int f = 0; f < 3; ++f) { L->offX[f] = o; o += (size_t)N * L->rows[f] * L->nx; }
    for (int f = 0; f < 3; ++f) { L->off5[f] = o; o += (size_t)N * L->rows[f]; }
    L->offAk = o;  o += (size_t)N * L->nx * L->nx;
    L->offABv = o; o += (size_t)N * L->nx * L->nv;
    L->offABw = o; o += (size_t)N * L->nx * L->nw;
    L->offAb5 = o; o += (size_t)N * L->nx;
    L->offS5 = o;  o += (size_t)(N + 1) * L->nx;
    L->offBv = o;  o += (size_t)L->nx * L->nv;
    L->offDv = o;  o += (size_t)L->ny * L->nv;
    L->offFv = o;  o += (size_t)L->nc * L->nv;
    L->blk_stride = (o + 15) & ~(size_t)15;
    const size_t n = (size_t)N * L->nv, nW = (size_t)N * L->nw;
    for (int f = 0; f < 3; ++f) {
        const size_t R = (size_t)N * L->rows[f];
        L->out_size[f * 4 + 0] = R * L->nx;
        L->out_size[f * 4 + 1] = R * n;
        L->out_size[f * 4 + 2] = R * nW;
        L->out_size[f * 4 + 3] = R;
    }
}

struct CondPtrs {
    const double *mats[20];     // device base pointers (per model stride = mat_size)
    size_t mat_size[20];
    double *blocks;
    double *out[12];
    const double *pack;         // per-model packed matrices in LDS order (mld_model::d_pack)
    size_t pack_len;
};

// C[m x n] = alpha * A[m x k] B[k x n] + beta * C0[m x n]   (all row-major, tiny) ; threads stride outputs
__device__ __forceinline__ void d_mm(double *C, const double *A, const double *B, int m, int k, int n, double alpha,
                                     const double *C0, double beta, int tid, int nt)
{
    for (int e = tid; e < m * n; e += nt) {
        const int i = e / n, j = e - i * n;
        double s = 0.0;
        for (int p = 0; p < k; ++p) s += A[i * k + p] * B[p * n + j];
        C[e] = alpha * s + (C0 ? beta * C0[e] : 0.0);
    }
}

// One workgroup per (block index k, model).  Block k needs A^{k-1} (lag blocks), A^k and S5_k = sum_{j<k} A^j b5
// (x / constant columns of block-row k); each workgroup rebuilds them in LDS by k tiny products (nx <= 15) instead of
// waiting for a serial chain -- N x n_models workgroups, ~10 us, instead of n_models workgroups x N barriers.
#define COND_UNROLL _Pragma("unroll 8")
__global__ void __launch_bounds__(128) k_condense_blocks(CondLayout L, CondPtrs P)
{
    extern __shared__ double sm[];
    const int k = blockIdx.x, mdl = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
    double *S = P.blocks + (size_t)mdl * L.blk_stride;
    const int nx = L.nx, nv = L.nv, nw = L.nw, ny = L.ny, nc = L.nc;
    // all small system matrices of the model, packed in this order on the host: one sweep with 8 independent loads per thread
    {
        const double *g = P.pack + (size_t)mdl * P.pack_len;
        const int tot = (int)P.pack_len;
#pragma unroll 8
        for (int e = tid; e < tot; e += nt) sm[e] = g[e];
    }
    double *stage = sm;
    auto take = [&](int len) -> double * { double *r = stage; stage += len; return r; };
    const double *A = take(nx * nx), *B4 = take(nx * nw), *b5 = take(nx), *C = take(ny * nx), *D4 = take(ny * nw), *d5 = take(ny),
                 *E = take(nc * nx), *F4 = take(nc * nw), *f5 = take(nc), *G = take(nc * ny);
    double *Bv = take(nx * nv);            // [B1 B2 B3 0]   nx*nv
    double *Dv = take(ny * nv);            // [D1 D2 D3 0]   ny*nv
    double *Fv = take(nc * nv);            // [F1 F2 F3 Psi] nc*nv
    // LDS scratch
    double *Pk = stage;                    // A^k            nx*nx
    double *Pm = Pk + nx * nx;             // A^{k-1}        nx*nx
    double *Tm = Pm + nx * nx;             // scratch        nx*nx
    double *s5 = Tm + nx * nx;             // S5_k           nx
    double *t5 = s5 + nx;                  // scratch        nx
    double *ABv = t5 + nx;                 // A^{k-1} Bv     nx*nv
    double *ABw = ABv + nx * nv;           // A^{k-1} B4     nx*nw
    double *Lv = ABw + nx * nw;            // output block   ny*nv
    double *Lw = Lv + ny * nv;             //                ny*nw
    double *Lx = Lw + ny * nw;             // C A^k          ny*nx
    double *l5 = Lx + ny * nx;             // C S5 + d5      ny
    for (int e = tid; e < nx * nx; e += nt) { Pk[e] = (e / nx == e % nx) ? 1.0 : 0.0; Pm[e] = 0.0; }
    for (int e = tid; e < nx; e += nt) s5[e] = 0.0;
    __syncthreads();
    // A^k, A^{k-1} (mld_evolution_matrices.py:272) and S5_k = sum_{j<k} A^j b5 (:331-332).  The reference builds them by a
    // chain of k products; here (P, s) = (A^m, sum_{j<m} A^j b5) reaches m = k-1 by square-and-multiply on the bits
    // of k-1 -- doubling: (P P, s + P s), increment: (P A, s + P b5) -- i.e. <= 2 log2(k) tiny products instead of k.
    if (k >= 1) {
        const int e = k - 1;
        int top = 0;
        while ((e >> top) > 1) ++top;
        for (int bit = (e > 0 ? top : -1); bit >= 0; --bit) {
            if (bit != top) {                  // doubling (the leading bit is handled by the increment from m = 0)
                for (int q = tid; q < nx; q += nt) { double acc = 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) acc += Pk[q * nx + p] * s5[p]; t5[q] = s5[q] + acc; }
                for (int q = tid; q < nx * nx; q += nt) { const int i = q / nx, c = q - i * nx; double acc = 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) acc += Pk[i * nx + p] * Pk[p * nx + c]; Tm[q] = acc; }
                __syncthreads();
                for (int q = tid; q < nx * nx; q += nt) Pk[q] = Tm[q];
                for (int q = tid; q < nx; q += nt) s5[q] = t5[q];
                __syncthreads();
            }
            if ((e >> bit) & 1) {              // increment
                for (int q = tid; q < nx; q += nt) { double acc = 0.0; if (b5) COND_UNROLL for (int p = 0; p < nx; ++p) acc += Pk[q * nx + p] * b5[p]; t5[q] = s5[q] + acc; }
                for (int q = tid; q < nx * nx; q += nt) { const int i = q / nx, c = q - i * nx; double acc = 0.0; if (A) COND_UNROLL for (int p = 0; p < nx; ++p) acc += Pk[i * nx + p] * A[p * nx + c]; Tm[q] = acc; }
                __syncthreads();
                for (int q = tid; q < nx * nx; q += nt) Pk[q] = Tm[q];
                for (int q = tid; q < nx; q += nt) s5[q] = t5[q];
                __syncthreads();
            }
        }
        // now Pk = A^{k-1}, s5 = S5_{k-1}: one more increment gives A^k and S5_k, keeping A^{k-1} in Pm
        for (int q = tid; q < nx; q += nt) { double acc = 0.0; if (b5) COND_UNROLL for (int p = 0; p < nx; ++p) acc += Pk[q * nx + p] * b5[p]; t5[q] = s5[q] + acc; }
        for (int q = tid; q < nx * nx; q += nt) { const int i = q / nx, c = q - i * nx; double acc = 0.0; if (A) COND_UNROLL for (int p = 0; p < nx; ++p) acc += Pk[i * nx + p] * A[p * nx + c]; Tm[q] = acc; }
        __syncthreads();
        for (int q = tid; q < nx * nx; q += nt) { Pm[q] = Pk[q]; Pk[q] = Tm[q]; }
        for (int q = tid; q < nx; q += nt) s5[q] = t5[q];
        __syncthreads();
    }
    // lag blocks of index k: A^{k-1} [Bv | B4]  (k >= 1), diagonal terms for k == 0
    for (int e = tid; e < nx * nv; e += nt) {
        const int i = e / nv, c = e - i * nv;
        double acc = 0.0;
        if (k > 0) COND_UNROLL for (int p = 0; p < nx; ++p) acc += Pm[i * nx + p] * Bv[p * nv + c];
        ABv[e] = acc;
    }
    for (int e = tid; e < nx * nw; e += nt) {
        const int i = e / nw, c = e - i * nw;
        double acc = 0.0;
        if (k > 0 && B4) COND_UNROLL for (int p = 0; p < nx; ++p) acc += Pm[i * nx + p] * B4[p * nw + c];
        ABw[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < ny * nv; e += nt) {          // L = C Gamma + D   (:186-189)
        const int i = e / nv, c = e - i * nv;
        double acc = (k == 0) ? Dv[e] : 0.0;
        if (k > 0 && C) COND_UNROLL for (int p = 0; p < nx; ++p) acc += C[i * nx + p] * ABv[p * nv + c];
        Lv[e] = acc;
    }
    for (int e = tid; e < ny * nw; e += nt) {
        const int i = e / nw, c = e - i * nw;
        double acc = (k == 0 && D4) ? D4[e] : 0.0;
        if (k > 0 && C) COND_UNROLL for (int p = 0; p < nx; ++p) acc += C[i * nx + p] * ABw[p * nw + c];
        Lw[e] = acc;
    }
    for (int e = tid; e < ny * nx; e += nt) {
        const int i = e / nx, c = e - i * nx;
        double acc = 0.0;
        if (C) COND_UNROLL for (int p = 0; p < nx; ++p) acc += C[i * nx + p] * Pk[p * nx + c];
        Lx[e] = acc;
    }
    for (int i = tid; i < ny; i += nt) {
        double acc = 0.0;
        if (C) COND_UNROLL for (int p = 0; p < nx; ++p) acc += C[i * nx + p] * s5[p];
        l5[i] = acc + (d5 ? d5[i] : 0.0);
    }
    __syncthreads();
    // write the block store (state, output, constraint families)
    double *V0 = S + L.offV[0] + (size_t)k * nx * nv, *V1 = S + L.offV[1] + (size_t)k * ny * nv, *V2 = S + L.offV[2] + (size_t)k * nc * nv;
    double *W0 = S + L.offW[0] + (size_t)k * nx * nw, *W1 = S + L.offW[1] + (size_t)k * ny * nw, *W2 = S + L.offW[2] + (size_t)k * nc * nw;
    double *X0 = S + L.offX[0] + (size_t)k * nx * nx, *X1 = S + L.offX[1] + (size_t)k * ny * nx, *X2 = S + L.offX[2] + (size_t)k * nc * nx;
    double *c0 = S + L.off5[0] + (size_t)k * nx, *c1 = S + L.off5[1] + (size_t)k * ny, *c2 = S + L.off5[2] + (size_t)k * nc;
    for (int e = tid; e < nx * nv; e += nt) V0[e] = ABv[e];
    for (int e = tid; e < nx * nw; e += nt) W0[e] = ABw[e];
    for (int e = tid; e < nx * nx; e += nt) X0[e] = Pk[e];
    for (int e = tid; e < nx; e += nt) c0[e] = s5[e];
    for (int e = tid; e < ny * nv; e += nt) V1[e] = Lv[e];
    for (int e = tid; e < ny * nw; e += nt) W1[e] = Lw[e];
    for (int e = tid; e < ny * nx; e += nt) X1[e] = Lx[e];
    for (int e = tid; e < ny; e += nt) c1[e] = l5[e];
    // constraint family (:237-240):  H_v = E Gamma_v + F_v + G L_v ; H_w = -(E Gamma_w + F4 + G L_w)
    //                                H_x = -(E Phi + G L_x)        ; H_5 = f5 - (E Gamma_5 + G L_5)
    for (int e = tid; e < nc * nv; e += nt) {
        const int i = e / nv, c = e - i * nv;
        double acc = (k == 0) ? Fv[e] : 0.0;
        if (k > 0 && E) COND_UNROLL for (int p = 0; p < nx; ++p) acc += E[i * nx + p] * ABv[p * nv + c];
        if (G) COND_UNROLL for (int p = 0; p < ny; ++p) acc += G[i * ny + p] * Lv[p * nv + c];
        V2[e] = acc;
    }
    for (int e = tid; e < nc * nw; e += nt) {
        const int i = e / nw, c = e - i * nw;
        double acc = (k == 0 && F4) ? F4[e] : 0.0;
        if (k > 0 && E) COND_UNROLL for (int p = 0; p < nx; ++p) acc += E[i * nx + p] * ABw[p * nw + c];
        if (G) COND_UNROLL for (int p = 0; p < ny; ++p) acc += G[i * ny + p] * Lw[p * nw + c];
        W2[e] = -acc;
    }
    for (int e = tid; e < nc * nx; e += nt) {
        const int i = e / nx, c = e - i * nx;
        double acc = 0.0;
        if (E) COND_UNROLL for (int p = 0; p < nx; ++p) acc += E[i * nx + p] * Pk[p * nx + c];
        if (G) COND_UNROLL for (int p = 0; p < ny; ++p) acc += G[i * ny + p] * Lx[p * nx + c];
        X2[e] = -acc;
    }
    for (int i = tid; i < nc; i += nt) {
        double acc = 0.0;
        if (E) COND_UNROLL for (int p = 0; p < nx; ++p) acc += E[i * nx + p] * s5[p];
        if (G) COND_UNROLL for (int p = 0; p < ny; ++p) acc += G[i * ny + p] * l5[p];
        c2[i] = (f5 ? f5[i] : 0.0) - acc;
    }
}

// K1, one workgroup per MODEL (shapes whose N block sets fit LDS -- every BASELINE shape up to cfg4; k_condense_blocks above
// stays for the rest): the powers A^k and the affine sums S5_k of all k at once by parallel prefix doubling,
// P[h+b] = P[h] P[b], S5[h+b] = S5[h] + P[h] S5[b] for b = 1..h (log2 N rounds of independent tiny products instead of a
// chain per block), then every block product for every k in one wide phase and coalesced copies into the block store.
__global__ void __launch_bounds__(1024) k_condense_model(CondLayout L, CondPtrs P)
{
    extern __shared__ double sm[];
    const int mdl = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, N = L.N;
    const int split = gridDim.y, k0 = blockIdx.y, nk = k0 < N ? (N - 1 - k0) / split + 1 : 0;   // this workgroup's blocks: k = k0 + kk * split
    const int nx = L.nx, nv = L.nv, nw = L.nw, ny = L.ny, nc = L.nc, nn = nx * nx;
    double *S = P.blocks + (size_t)mdl * L.blk_stride;
    {
        const double *g = P.pack + (size_t)mdl * P.pack_len;
        const int tot = (int)P.pack_len;
        for (int e = tid; e < tot; e += nt) sm[e] = g[e];
    }
    double *stage = sm;
    auto take = [&](int len) -> double * { double *r = stage; stage += len; return r; };
    const double *A = take(nn), *B4 = take(nx * nw), *b5 = take(nx), *C = take(ny * nx), *D4 = take(ny * nw), *d5 = take(ny),
                 *E = take(nc * nx), *F4 = take(nc * nw), *f5 = take(nc), *G = take(nc * ny);
    const double *Bv = take(nx * nv), *Dv = take(ny * nv), *Fv = take(nc * nv);
    const int nkm = (N - 1) / split + 1;
    double *Pw = take(N * nn), *S5 = take(N * nx), *ABv = take(nkm * nx * nv), *ABw = take(nkm * nx * nw), *Lv = take(nkm * ny * nv),
           *Lw = take(nkm * ny * nw), *Lx = take(nkm * ny * nx), *l5 = take(nkm * ny);
    __syncthreads();
    for (int e = tid; e < nn; e += nt) { Pw[e] = (e / nx == e % nx) ? 1.0 : 0.0; if (N > 1) Pw[nn + e] = A[e]; }
    for (int e = tid; e < nx; e += nt) { S5[e] = 0.0; if (N > 1) S5[nx + e] = b5[e]; }
    __syncthreads();
    for (int h = 1; h < N - 1; h <<= 1) {
        const int cnt = (2 * h < N - 1 ? 2 * h : N - 1) - h;
        const double *Ph = Pw + (size_t)h * nn;
        for (int e = tid; e < cnt * nn; e += nt) {
            const int kk = e / nn, q = e - kk * nn, r = q / nx, c = q - r * nx;
            const double *Pb = Pw + (size_t)(kk + 1) * nn;
            double a = 0.0;
            COND_UNROLL for (int p = 0; p < nx; ++p) a += Ph[r * nx + p] * Pb[p * nx + c];
            Pw[(size_t)(h + 1 + kk) * nn + q] = a;
        }
        for (int e = tid; e < cnt * nx; e += nt) {
            const int kk = e / nx, r = e - kk * nx;
            const double *sb = S5 + (size_t)(kk + 1) * nx;
            double a = S5[h * nx + r];
            COND_UNROLL for (int p = 0; p < nx; ++p) a += Ph[r * nx + p] * sb[p];
            S5[(size_t)(h + 1 + kk) * nx + r] = a;
        }
        __syncthreads();
    }
    // lag blocks A^{k-1} [Bv | B4] (zero for k = 0), x / constant columns of the output family
    for (int e = tid; e < nk * nx * nv; e += nt) {
        const int kk = e / (nx * nv), k = k0 + kk * split, q = e - kk * nx * nv, r = q / nv, c = q - r * nv;
        double a = 0.0;
        if (k > 0) { const double *Pm = Pw + (size_t)(k - 1) * nn + r * nx; COND_UNROLL for (int p = 0; p < nx; ++p) a += Pm[p] * Bv[p * nv + c]; }
        ABv[e] = a;
    }
    for (int e = tid; e < nk * nx * nw; e += nt) {
        const int kk = e / (nx * nw), k = k0 + kk * split, q = e - kk * nx * nw, r = q / nw, c = q - r * nw;
        double a = 0.0;
        if (k > 0) { const double *Pm = Pw + (size_t)(k - 1) * nn + r * nx; COND_UNROLL for (int p = 0; p < nx; ++p) a += Pm[p] * B4[p * nw + c]; }
        ABw[e] = a;
    }
    for (int e = tid; e < nk * ny * nx; e += nt) {
        const int kk = e / (ny * nx), k = k0 + kk * split, q = e - kk * ny * nx, r = q / nx, c = q - r * nx;
        const double *Pk = Pw + (size_t)k * nn;
        double a = 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += C[r * nx + p] * Pk[p * nx + c];
        Lx[e] = a;
    }
    for (int e = tid; e < nk * ny; e += nt) {
        const int kk = e / ny, k = k0 + kk * split, r = e - kk * ny;
        double a = d5[r];
        COND_UNROLL for (int p = 0; p < nx; ++p) a += C[r * nx + p] * S5[k * nx + p];
        l5[e] = a;
    }
    __syncthreads();
    for (int e = tid; e < nk * ny * nv; e += nt) {          // L = C Gamma + D   (:186-189)
        const int kk = e / (ny * nv), k = k0 + kk * split, q = e - kk * ny * nv, r = q / nv, c = q - r * nv;
        const double *X = ABv + (size_t)kk * nx * nv + c;
        double a = k == 0 ? Dv[q] : 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += C[r * nx + p] * X[p * nv];
        Lv[e] = a;
    }
    for (int e = tid; e < nk * ny * nw; e += nt) {
        const int kk = e / (ny * nw), k = k0 + kk * split, q = e - kk * ny * nw, r = q / nw, c = q - r * nw;
        const double *X = ABw + (size_t)kk * nx * nw + c;
        double a = k == 0 ? D4[q] : 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += C[r * nx + p] * X[p * nw];
        Lw[e] = a;
    }
    __syncthreads();
    // block store: block k of a family is one contiguous chunk, in the LDS layout [r][c]
    for (int e = tid; e < nk * nx * nv; e += nt) { const int kk = e / (nx * nv); S[L.offV[0] + (size_t)(k0 + kk * split) * nx * nv + (e - kk * nx * nv)] = ABv[e]; }
    for (int e = tid; e < nk * nx * nw; e += nt) { const int kk = e / (nx * nw); S[L.offW[0] + (size_t)(k0 + kk * split) * nx * nw + (e - kk * nx * nw)] = ABw[e]; }
    for (int e = tid; e < nk * nn; e += nt) { const int kk = e / nn, k = k0 + kk * split; S[L.offX[0] + (size_t)k * nn + (e - kk * nn)] = Pw[(size_t)k * nn + (e - kk * nn)]; }
    for (int e = tid; e < nk * nx; e += nt) { const int kk = e / nx, k = k0 + kk * split; S[L.off5[0] + (size_t)k * nx + (e - kk * nx)] = S5[(size_t)k * nx + (e - kk * nx)]; }
    for (int e = tid; e < nk * ny * nv; e += nt) { const int kk = e / (ny * nv); S[L.offV[1] + (size_t)(k0 + kk * split) * ny * nv + (e - kk * ny * nv)] = Lv[e]; }
    for (int e = tid; e < nk * ny * nw; e += nt) { const int kk = e / (ny * nw); S[L.offW[1] + (size_t)(k0 + kk * split) * ny * nw + (e - kk * ny * nw)] = Lw[e]; }
    for (int e = tid; e < nk * ny * nx; e += nt) { const int kk = e / (ny * nx); S[L.offX[1] + (size_t)(k0 + kk * split) * ny * nx + (e - kk * ny * nx)] = Lx[e]; }
    for (int e = tid; e < nk * ny; e += nt) { const int kk = e / ny; S[L.off5[1] + (size_t)(k0 + kk * split) * ny + (e - kk * ny)] = l5[e]; }
    // constraint family (:237-240):  H_v = E Gamma_v + F_v + G L_v ; H_w = -(E Gamma_w + F4 + G L_w)
    //                                H_x = -(E Phi + G L_x)        ; H_5 = f5 - (E Gamma_5 + G L_5)
    for (int e = tid; e < nk * nc * nv; e += nt) {
        const int kk = e / (nc * nv), k = k0 + kk * split, q = e - kk * nc * nv, r = q / nv, c = q - r * nv;
        const double *X = ABv + (size_t)kk * nx * nv + c, *Y = Lv + (size_t)kk * ny * nv + c;
        double a = k == 0 ? Fv[q] : 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += E[r * nx + p] * X[p * nv];
        COND_UNROLL for (int p = 0; p < ny; ++p) a += G[r * ny + p] * Y[p * nv];
        S[L.offV[2] + (size_t)k * nc * nv + q] = a;
    }
    for (int e = tid; e < nk * nc * nw; e += nt) {
        const int kk = e / (nc * nw), k = k0 + kk * split, q = e - kk * nc * nw, r = q / nw, c = q - r * nw;
        const double *X = ABw + (size_t)kk * nx * nw + c, *Y = Lw + (size_t)kk * ny * nw + c;
        double a = k == 0 ? F4[q] : 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += E[r * nx + p] * X[p * nw];
        COND_UNROLL for (int p = 0; p < ny; ++p) a += G[r * ny + p] * Y[p * nw];
        S[L.offW[2] + (size_t)k * nc * nw + q] = -a;
    }
    for (int e = tid; e < nk * nc * nx; e += nt) {
        const int kk = e / (nc * nx), k = k0 + kk * split, q = e - kk * nc * nx, r = q / nx, c = q - r * nx;
        const double *X = Pw + (size_t)k * nn + c, *Y = Lx + (size_t)kk * ny * nx + c;
        double a = 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += E[r * nx + p] * X[p * nx];
        COND_UNROLL for (int p = 0; p < ny; ++p) a += G[r * ny + p] * Y[p * nx];
        S[L.offX[2] + (size_t)k * nc * nx + q] = -a;
    }
    for (int e = tid; e < nk * nc; e += nt) {
        const int kk = e / nc, k = k0 + kk * split, r = e - kk * nc;
        double a = 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += E[r * nx + p] * S5[k * nx + p];
        COND_UNROLL for (int p = 0; p < ny; ++p) a += G[r * ny + p] * l5[kk * ny + p];
        S[L.off5[2] + (size_t)k * nc + r] = f5[r] - a;
    }
}

static size_t condense_model_lds(const CondLayout &L, size_t pack_len, int split)
{
    const size_t N = L.N, nkm = (N - 1) / split + 1;
    return sizeof(double) * (pack_len + N * ((size_t)L.nx * L.nx + L.nx) + nkm * ((size_t)(L.nx + L.ny) * (L.nv + L.nw) + (size_t)L.ny * L.nx + L.ny) + 16);
}

#define COND_ROWS_PER_WG 8
// one workgroup per (model, COND_ROWS_PER_WG consecutive output rows): writes those rows of the four matrices of the family
__global__ void __launch_bounds__(256) k_condense_scatter(CondLayout L, CondPtrs P, int rows_total, int skip_vw)
{
    const int mdl = blockIdx.y;
    for (int R0 = blockIdx.x * COND_ROWS_PER_WG; R0 < rows_total && R0 < (blockIdx.x + 1) * COND_ROWS_PER_WG; ++R0) {
    int R = R0;                         // global row over the three families
    int f = 0;
    const int N = L.N;
    if (R >= N * L.rows[0]) { R -= N * L.rows[0]; f = 1; if (R >= N * L.rows[1]) { R -= N * L.rows[1]; f = 2; } }
    const int rf = L.rows[f];
    const int i = R / rf, r = R - i * rf;
    const double *S = P.blocks + (size_t)mdl * L.blk_stride;
    const int nv = L.nv, nw = L.nw, nx = L.nx;
    const int tid = threadIdx.x, nt = blockDim.x;
    const float inv_nv = nv ? 1.0f / (float)nv : 0.0f, inv_nw = nw ? 1.0f / (float)nw : 0.0f;
    const size_t n = (size_t)N * nv, nW = (size_t)N * nw;
    // v part: block (i,j) = blkV[f][i-j] for j <= i, zero above the diagonal
    if (P.out[f * 4 + 1] && !skip_vw) {
        double *o = P.out[f * 4 + 1] + (size_t)mdl * L.out_size[f * 4 + 1] + (size_t)R * n;
        const double *bv = S + L.offV[f];
        const int lim = (i + 1) * nv;
        for (int col0 = tid; col0 < (int)n; col0 += 4 * nt) {      // 4 independent loads in flight per thread
            double v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int col = col0 + t * nt;
                v[t] = 0.0;
                if (col < lim) {
                    int j = __float2int_rz(((float)col + 0.5f) * inv_nv), c = col - j * nv;   // col / nv without an integer divide
                    if (c < 0) { --j; c += nv; } else if (c >= nv) { ++j; c -= nv; }
                    v[t] = bv[((size_t)(i - j) * rf + r) * nv + c];
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) { const int col = col0 + t * nt; if (col < (int)n) o[col] = v[t]; }
        }
    }
    if (P.out[f * 4 + 2] && !skip_vw) {
        double *o = P.out[f * 4 + 2] + (size_t)mdl * L.out_size[f * 4 + 2] + (size_t)R * nW;
        const double *bw = S + L.offW[f];
        const int lim = (i + 1) * nw;
        for (int col = tid; col < (int)nW; col += nt) {
            double v = 0.0;
            if (col < lim) {
                int j = __float2int_rz(((float)col + 0.5f) * inv_nw), c = col - j * nw;
                if (c < 0) { --j; c += nw; } else if (c >= nw) { ++j; c -= nw; }
                v = bw[((size_t)(i - j) * rf + r) * nw + c];
            }
            o[col] = v;
        }
    }
    if (P.out[f * 4 + 0]) {
        double *o = P.out[f * 4 + 0] + (size_t)mdl * L.out_size[f * 4 + 0] + (size_t)R * nx;
        const double *bx = S + L.offX[f] + ((size_t)i * rf + r) * nx;
        for (int c = tid; c < nx; c += nt) o[c] = bx[c];
    }
    if (P.out[f * 4 + 3] && tid == 0)
        P.out[f * 4 + 3][(size_t)mdl * L.out_size[f * 4 + 3] + R] = S[L.off5[f] + (size_t)i * rf + r];
    }
}

// The input-map matrices (Gamma_v/Gamma_w, L_v/L_w, H_v/H_w: 98 % of the bytes) as flat write streams: a workgroup owns
// COND_FLAT doubles of one whole allocation (all models), so every chunk starts 16-byte aligned although rows (odd
// length) and models do not; a thread writes four double2 slots 256 slots apart (each wave store = 1 KiB contiguous).
// The (model, row, block-column) of a slot come from one integer division per thread, then advance incrementally.
#define COND_FLAT 2048
struct FlatJob { void *out; const double *blk_off_dummy; unsigned total; unsigned per_model; int rows; int width; int bw; int fam; int is_w; unsigned first_block; };
struct FlatJobs { FlatJob j[12]; int n; };   // v / w (Toeplitz lookups) and x / constant columns (plain copies of the block store) of the three families

// OutT = double (the reference's layout and dtype) or float (mld_condense_f32: the same fp64 block arithmetic, materialised in fp32 --
// half the bytes of the write stream that bounds this kernel)
template <typename OutT>
__global__ void __launch_bounds__(256) k_condense_flat(CondLayout L, CondPtrs P, FlatJobs J)
{
    constexpr int EPT = 16 / (int)sizeof(OutT);          // elements per 16-byte lane store: 2 doubles or 4 floats
    constexpr unsigned SLOT = 256u * EPT;                 // elements one workgroup store instruction covers
    constexpr int NSLOT = COND_FLAT / (int)SLOT * (sizeof(OutT) == 8 ? 1 : 2);     // a chunk is COND_FLAT doubles = 16 KB in either type
    constexpr unsigned CHUNK = SLOT * NSLOT;
    int a = 0;
    while (a + 1 < J.n && blockIdx.x >= J.j[a + 1].first_block) ++a;
    const FlatJob jb = J.j[a];
    const unsigned chunk0 = (blockIdx.x - jb.first_block) * CHUNK;
    const int rf = L.rows[jb.fam], bw = jb.bw, width = jb.width;
    const size_t boff = jb.is_w == 0 ? L.offV[jb.fam] : (jb.is_w == 1 ? L.offW[jb.fam] : (jb.is_w == 2 ? L.offX[jb.fam] : L.off5[jb.fam]));
    typedef OutT vec_t __attribute__((ext_vector_type(EPT)));
    OutT *const out = (OutT *)jb.out;
    if (jb.is_w >= 2) {   // x / constant columns: the block store already has the output layout per model -> plain copy
#pragma unroll
        for (int q = 0; q < NSLOT; ++q) {
            const unsigned E = chunk0 + (unsigned)EPT * (threadIdx.x + 256u * q);
            if (E >= jb.total) break;
            OutT v[EPT];
#pragma unroll
            for (int h = 0; h < EPT; ++h) {
                const unsigned Eh = E + h;
                double val = 0.0;
                if (Eh < jb.total) { const unsigned mdl = Eh / jb.per_model, e = Eh - mdl * jb.per_model; val = P.blocks[(size_t)mdl * L.blk_stride + boff + e]; }
                v[h] = (OutT)val;
            }
            if (E + EPT <= jb.total) { vec_t w; for (int h = 0; h < EPT; ++h) w[h] = v[h]; *(vec_t *)(out + E) = w; }
            else for (int h = 0; h < EPT && E + h < jb.total; ++h) out[E + h] = v[h];
        }
        return;
    }
    const unsigned uw = (unsigned)width, ubw = (unsigned)bw, urf = (unsigned)rf, rows = (unsigned)jb.rows;
    // position of the thread's first element: one set of divisions, then incremental
    unsigned E = chunk0 + (unsigned)EPT * threadIdx.x;
    if (E >= jb.total) return;
    unsigned mdl = E / jb.per_model, e = E - mdl * jb.per_model;
    unsigned R = e / uw, col = e - R * uw;
    unsigned i = R / urf, r = R - i * urf;
    unsigned jc = col / ubw, c = col - jc * ubw;
    const double *blk = P.blocks + (size_t)mdl * L.blk_stride + boff;
#pragma unroll
    for (int q = 0; q < NSLOT; ++q) {
        OutT v[EPT];
        // elements E .. E + EPT - 1: a running copy of the position advances by one element at a time
        unsigned c1 = c, jc1 = jc, col1 = col, r1 = r, i1 = i, R1 = R;
        const double *blk1 = blk;
#pragma unroll
        for (int h = 0; h < EPT; ++h) {
            v[h] = (E + h < jb.total && jc1 <= i1) ? (OutT)blk1[((size_t)(i1 - jc1) * urf + r1) * ubw + c1] : (OutT)0;
            ++c1; ++col1;
            if (c1 == ubw) { c1 = 0; ++jc1; }
            if (col1 == uw) { col1 = 0; c1 = 0; jc1 = 0; ++R1; ++r1; if (r1 == urf) { r1 = 0; ++i1; } if (R1 == rows) { R1 = 0; r1 = 0; i1 = 0; blk1 += L.blk_stride; } }
        }
        if (E + EPT <= jb.total) { vec_t w; for (int h = 0; h < EPT; ++h) w[h] = v[h]; *(vec_t *)(out + E) = w; }
        else for (int h = 0; h < EPT && E + h < jb.total; ++h) out[E + h] = v[h];
        // advance by one slot
        E += SLOT;
        if (E >= jb.total) break;
        col += SLOT;
        while (col >= uw) { col -= uw; ++R; ++r; if (r == urf) { r = 0; ++i; } if (R == rows) { R = 0; r = 0; i = 0; ++mdl; blk += L.blk_stride; } }
        jc = col / ubw; c = col - jc * ubw;
    }
}

// Time-varying horizon (mld_numeric_tilde, models/mld_model.py:1210-1227; the time-varying branch of
// mld_evolution_matrices.py:265-272): step k of the horizon has its own model, so block (i,j) of an input map is
// A_{i-1} ... A_{j+1} B_j -- a function of both indices, not of i-j, and there is no block store to share.  One
// workgroup owns block-row i of all twelve matrices of one horizon: it walks j = i .. 0 with Q = A_{i-1} ... A_{j+1}
// kept in LDS (one nx x nx product per column block), so successive iterations extend the same output rows from right
// to left and the rows above the diagonal are zero-filled by the same workgroup.  pack holds n_sets x N step models.
#ifndef COND_TV_JB
#define COND_TV_JB 8
#endif
#define COND_TV_PF 4
__global__ void __launch_bounds__(256) k_condense_tv(CondLayout L, CondPtrs P)
{
    extern __shared__ double sm[];
    const int N = L.N, i = N - 1 - (int)blockIdx.y, set = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;   // the longest block-rows of all horizons are dispatched first
    const int nx = L.nx, nv = L.nv, nw = L.nw, ny = L.ny, nc = L.nc;
    const int tot = (int)P.pack_len;
    const double *gset = P.pack + (size_t)set * N * P.pack_len;
    {
        const double *g = gset + (size_t)i * P.pack_len;
#pragma unroll 8
        for (int e = tid; e < tot; e += nt) sm[e] = g[e];
    }
    double *stage = sm;
    auto take = [&](int len) -> double * { double *r = stage; stage += len; return r; };
    take(nx * nx); take(nx * nw); take(nx);                   // A_i, B4_i, b5_i act on step i+1: not used by block-row i
    const double *C = take(ny * nx), *D4 = take(ny * nw), *d5 = take(ny), *E = take(nc * nx), *F4 = take(nc * nw), *f5 = take(nc),
                 *G = take(nc * ny);
    const int oB4 = nx * nx, ob5 = oB4 + nx * nw, oBv = (int)(stage - sm);
    take(nx * nv);
    const double *Dv = take(ny * nv), *Fv = take(nc * nv);
    double *Q = take(nx * nx), *Tq = take(nx * nx), *Aj = take(nx * nx), *B4j = take(nx * nw), *b5j = take(nx), *Bj = take(nx * nv);   // Aj..Bj contiguous: [A B4 b5 | Bv] of step j
    double *X = take(COND_TV_JB * nx * nv), *Xw = take(COND_TV_JB * nx * nw), *Lb = take(COND_TV_JB * ny * nv), *Lbw = take(COND_TV_JB * ny * nw), *s5 = take(nx), *t5 = take(nx);
    double *Lx = take(ny * nx), *l5 = take(ny);
    for (int e = tid; e < nx * nx; e += nt) Q[e] = (e / nx == e % nx) ? 1.0 : 0.0;
    for (int e = tid; e < nx; e += nt) s5[e] = 0.0;
    const size_t n = (size_t)N * nv, nW = (size_t)N * nw;
    double *oV[3], *oW[3];
    for (int f = 0; f < 3; ++f) {
        oV[f] = P.out[f * 4 + 1] ? P.out[f * 4 + 1] + (size_t)set * L.out_size[f * 4 + 1] + (size_t)i * L.rows[f] * n : nullptr;
        oW[f] = P.out[f * 4 + 2] ? P.out[f * 4 + 2] + (size_t)set * L.out_size[f * 4 + 2] + (size_t)i * L.rows[f] * nW : nullptr;
    }
    __syncthreads();
    // step j's dynamics [A B4 b5 | Bv] travel global -> registers -> LDS one iteration ahead of their use, so the load
    // latency hides behind the products of step j+1 (three barriers per column block)
    const int nA = nx * nx + nx * nw + nx, nS = nA + nx * nv;
    const bool pf = nS <= COND_TV_PF * 256;
    double reg[COND_TV_PF];
    auto fetch = [&](int j) {
        const double *g = gset + (size_t)j * P.pack_len;
#pragma unroll
        for (int q = 0; q < COND_TV_PF; ++q) { const int e = tid + q * 256; reg[q] = e < nS ? g[e < nA ? e : oBv + (e - nA)] : 0.0; }
    };
    if (pf && i > 0) fetch(i - 1);
    // column blocks are produced COND_TV_JB at a time (the chain over j is serial) and written together, so that a row
    // segment of one write phase is COND_TV_JB * nv contiguous doubles
    for (int jhi = i; jhi >= 0; jhi -= COND_TV_JB) {
        const int jlo = jhi - COND_TV_JB + 1 > 0 ? jhi - COND_TV_JB + 1 : 0, nj = jhi - jlo + 1;
        for (int j = jhi; j >= jlo; --j) {
            const bool diag = (j == i);
            const int sl = j - jlo;
            double *Xs = X + sl * nx * nv, *Xws = Xw + sl * nx * nw, *Ls = Lb + sl * ny * nv, *Lws = Lbw + sl * ny * nw;
            if (!diag) {
                if (pf) {
#pragma unroll
                    for (int q = 0; q < COND_TV_PF; ++q) { const int e = tid + q * 256; if (e < nS) Aj[e] = reg[q]; }
                } else {
                    const double *g = gset + (size_t)j * P.pack_len;
                    for (int e = tid; e < nS; e += nt) Aj[e] = g[e < nA ? e : oBv + (e - nA)];
                }
                __syncthreads();
                if (pf && j > 0) fetch(j - 1);
                for (int e = tid; e < nx * nv; e += nt) { const int r = e / nv, c = e - r * nv; double a = 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) a += Q[r * nx + p] * Bj[p * nv + c]; Xs[e] = a; }
                for (int e = tid; e < nx * nw; e += nt) { const int r = e / nw, c = e - r * nw; double a = 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) a += Q[r * nx + p] * B4j[p * nw + c]; Xws[e] = a; }
                for (int e = tid; e < nx; e += nt) { double a = 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) a += Q[e * nx + p] * b5j[p]; t5[e] = s5[e] + a; }
                for (int e = tid; e < nx * nx; e += nt) { const int r = e / nx, c = e - r * nx; double a = 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) a += Q[r * nx + p] * Aj[p * nx + c]; Tq[e] = a; }
            } else {
                for (int e = tid; e < nx * nv; e += nt) Xs[e] = 0.0;
                for (int e = tid; e < nx * nw; e += nt) Xws[e] = 0.0;
            }
            __syncthreads();
            if (!diag) {
                for (int e = tid; e < nx * nx; e += nt) Q[e] = Tq[e];
                for (int e = tid; e < nx; e += nt) s5[e] = t5[e];
            }
            for (int e = tid; e < ny * nv; e += nt) { const int r = e / nv, c = e - r * nv; double a = diag ? Dv[e] : 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) a += C[r * nx + p] * Xs[p * nv + c]; Ls[e] = a; }
            for (int e = tid; e < ny * nw; e += nt) { const int r = e / nw, c = e - r * nw; double a = diag ? D4[e] : 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) a += C[r * nx + p] * Xws[p * nw + c]; Lws[e] = a; }
            // (the next step's first barrier orders this phase before the products that read Q)
        }
        __syncthreads();
        const int Wv = nj * nv, Ww = nj * nw;
        const bool hasdiag = (jhi == i);                      // the diagonal block sits in the last slot of the first group
        if (oV[0]) for (int e = tid; e < nx * Wv; e += nt) { const int r = e / Wv, cc = e - r * Wv, sl = cc / nv, c = cc - sl * nv; oV[0][(size_t)r * n + (size_t)jlo * nv + cc] = X[sl * nx * nv + r * nv + c]; }
        if (oW[0]) for (int e = tid; e < nx * Ww; e += nt) { const int r = e / Ww, cc = e - r * Ww, sl = cc / nw, c = cc - sl * nw; oW[0][(size_t)r * nW + (size_t)jlo * nw + cc] = Xw[sl * nx * nw + r * nw + c]; }
        if (oV[1]) for (int e = tid; e < ny * Wv; e += nt) { const int r = e / Wv, cc = e - r * Wv, sl = cc / nv, c = cc - sl * nv; oV[1][(size_t)r * n + (size_t)jlo * nv + cc] = Lb[sl * ny * nv + r * nv + c]; }
        if (oW[1]) for (int e = tid; e < ny * Ww; e += nt) { const int r = e / Ww, cc = e - r * Ww, sl = cc / nw, c = cc - sl * nw; oW[1][(size_t)r * nW + (size_t)jlo * nw + cc] = Lbw[sl * ny * nw + r * nw + c]; }
        if (oV[2]) for (int e = tid; e < nc * Wv; e += nt) {
            const int r = e / Wv, cc = e - r * Wv, sl = cc / nv, c = cc - sl * nv;
            const double *Xs = X + sl * nx * nv, *Ls = Lb + sl * ny * nv;
            double a = (hasdiag && sl == nj - 1) ? Fv[r * nv + c] : 0.0;
            COND_UNROLL for (int p = 0; p < nx; ++p) a += E[r * nx + p] * Xs[p * nv + c];
            COND_UNROLL for (int p = 0; p < ny; ++p) a += G[r * ny + p] * Ls[p * nv + c];
            oV[2][(size_t)r * n + (size_t)jlo * nv + cc] = a;
        }
        if (oW[2]) for (int e = tid; e < nc * Ww; e += nt) {
            const int r = e / Ww, cc = e - r * Ww, sl = cc / nw, c = cc - sl * nw;
            const double *Xs = Xw + sl * nx * nw, *Ls = Lbw + sl * ny * nw;
            double a = (hasdiag && sl == nj - 1) ? F4[r * nw + c] : 0.0;
            COND_UNROLL for (int p = 0; p < nx; ++p) a += E[r * nx + p] * Xs[p * nw + c];
            COND_UNROLL for (int p = 0; p < ny; ++p) a += G[r * ny + p] * Ls[p * nw + c];
            oW[2][(size_t)r * nW + (size_t)jlo * nw + cc] = -a;
        }
        __syncthreads();
    }
    // x / constant columns of block-row i: Q = A_{i-1} ... A_0, s5 = sum_j A_{i-1} ... A_{j+1} b5_j
    for (int e = tid; e < ny * nx; e += nt) { const int r = e / nx, c = e - r * nx; double a = 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) a += C[r * nx + p] * Q[p * nx + c]; Lx[e] = a; }
    for (int e = tid; e < ny; e += nt) { double a = 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) a += C[e * nx + p] * s5[p]; l5[e] = a + d5[e]; }
    __syncthreads();
    double *oX[3], *o5[3];
    for (int f = 0; f < 3; ++f) {
        oX[f] = P.out[f * 4 + 0] ? P.out[f * 4 + 0] + (size_t)set * L.out_size[f * 4 + 0] + (size_t)i * L.rows[f] * nx : nullptr;
        o5[f] = P.out[f * 4 + 3] ? P.out[f * 4 + 3] + (size_t)set * L.out_size[f * 4 + 3] + (size_t)i * L.rows[f] : nullptr;
    }
    if (oX[0]) for (int e = tid; e < nx * nx; e += nt) oX[0][e] = Q[e];
    if (o5[0]) for (int e = tid; e < nx; e += nt) o5[0][e] = s5[e];
    if (oX[1]) for (int e = tid; e < ny * nx; e += nt) oX[1][e] = Lx[e];
    if (o5[1]) for (int e = tid; e < ny; e += nt) o5[1][e] = l5[e];
    if (oX[2]) for (int e = tid; e < nc * nx; e += nt) {
        const int r = e / nx, c = e - r * nx;
        double a = 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += E[r * nx + p] * Q[p * nx + c];
        COND_UNROLL for (int p = 0; p < ny; ++p) a += G[r * ny + p] * Lx[p * nx + c];
        oX[2][e] = -a;
    }
    if (o5[2]) for (int e = tid; e < nc; e += nt) {
        double a = 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += E[e * nx + p] * s5[p];
        COND_UNROLL for (int p = 0; p < ny; ++p) a += G[e * ny + p] * l5[p];
        o5[2][e] = f5[e] - a;
    }
    // structural zeros right of the diagonal block
    for (int f = 0; f < 3; ++f) {
        const int rf = L.rows[f];
        const int zv = (N - 1 - i) * nv, zw = (N - 1 - i) * nw;
        if (oV[f]) for (int e = tid; e < rf * zv; e += nt) { const int r = e / zv, c = e - r * zv; oV[f][(size_t)r * n + (size_t)(i + 1) * nv + c] = 0.0; }
        if (oW[f]) for (int e = tid; e < rf * zw; e += nt) { const int r = e / zw, c = e - r * zw; oW[f][(size_t)r * nW + (size_t)(i + 1) * nw + c] = 0.0; }
    }
}

// ---- time-varying horizons, wide variant: the only serial part -- the products Q(i,j) = A_{i-1} ... A_{j+1} -- is split off.
// k_tv_chain: one workgroup per horizon, a wave per column chain j (Q(i+1,j) = A_i Q(i,j), wave-private ping-pong in LDS, no
// block barrier) writes all Q(i,j) (triangular, N(N+1)/2 x nx x nx: ~3 % of the output bytes) and the affine chain
// s5(i+1) = A_i s5(i) + b5_i.  k_tv_rows: one workgroup per (horizon, block-row i) then has no dependent chain at all:
// X = Q(i,j) B_j for every j at once into LDS, L = C X + D, and every output row is produced by one wave as ONE contiguous
// row (filled part + structural zeros), the constraint rows two at a time with the accumulators of a whole row in registers.
#define TV_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
__device__ __forceinline__ int tv_tri(int i) { return i * (i + 1) / 2; }

__global__ void __launch_bounds__(1024) k_tv_chain(CondLayout L, CondPtrs P, double *Qbuf, double *S5buf)
{
    extern __shared__ double sm[];
    const int set = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nwv = nt >> 6;
    const int N = L.N, nx = L.nx, nn = nx * nx, ob5 = nn + nx * L.nw;
    const double *gset = P.pack + (size_t)set * N * P.pack_len;
    double *As = sm, *b5s = As + (size_t)N * nn, *Qw = b5s + (size_t)N * nx + (size_t)wave * 2 * nn;
    for (int e = tid; e < N * nn; e += nt) { const int i = e / nn; As[e] = gset[(size_t)i * P.pack_len + (e - i * nn)]; }
    for (int e = tid; e < N * nx; e += nt) { const int i = e / nx; b5s[e] = gset[(size_t)i * P.pack_len + ob5 + (e - i * nx)]; }
    __syncthreads();
    double *qg = Qbuf + (size_t)set * tv_tri(N) * nn;
    double *sg = S5buf + (size_t)set * N * nx;
    // chains in descending length: v = 0 the affine chain (N-1 steps), v = jj + 1 the chain of column jj (N-1-jj steps; jj = j + 1,
    // jj = 0: the chain of Phi_x); dealt to the waves back and forth so that every wave gets about the same number of steps
    for (int k = 0; k * nwv <= N; ++k) {
        const int v = k * nwv + ((k & 1) ? nwv - 1 - wave : wave);
        if (v > N) continue;
        const int jj = v == 0 ? N : v - 1;
        double *qa = Qw, *qb = Qw + nn;
        if (jj == N) {
            for (int e = lane; e < nx; e += 64) { qa[e] = 0.0; sg[e] = 0.0; }
            TV_WSYNC();
            for (int i = 0; i + 1 < N; ++i) {
                const double *A = As + (size_t)i * nn;
                for (int e = lane; e < nx; e += 64) {
                    double a = b5s[i * nx + e];
                    COND_UNROLL for (int p = 0; p < nx; ++p) a += A[e * nx + p] * qa[p];
                    qb[e] = a; sg[(size_t)(i + 1) * nx + e] = a;
                }
                TV_WSYNC();
                double *t = qa; qa = qb; qb = t;
            }
            continue;
        }
        for (int e = lane; e < nn; e += 64) { const double v = (e / nx == e % nx) ? 1.0 : 0.0; qa[e] = v; qg[(size_t)(tv_tri(jj) + jj) * nn + e] = v; }
        TV_WSYNC();
        for (int i = jj; i + 1 < N; ++i) {
            const double *A = As + (size_t)i * nn;
            for (int e = lane; e < nn; e += 64) {
                const int r = e / nx, c = e - r * nx;
                double a = 0.0;
                COND_UNROLL for (int p = 0; p < nx; ++p) a += A[r * nx + p] * qa[p * nx + c];
                qb[e] = a; qg[(size_t)(tv_tri(i + 1) + jj) * nn + e] = a;
            }
            TV_WSYNC();
            double *t = qa; qa = qb; qb = t;
        }
    }
}

// one constraint-row pair (or one row) of block-row i: out = sign * (F(diag) + E X + G Lr), then zeros up to the full width
template <int TV_KC>
__device__ __forceinline__ void tv_hrows(double *o0, double *o1, const double *E0, const double *E1, const double *G0, const double *G1,
                                         const double *F0, const double *F1, const double *X, const double *Lr, int nx, int ny, int ld,
                                         int W, int full, int dcol, int bw, double sign, int lane)
{
    double a0[TV_KC], a1[TV_KC];
#pragma unroll
    for (int k = 0; k < TV_KC; ++k) {
        const int col = lane + 64 * k;
        const bool dg = col >= dcol && col < W;
        a0[k] = dg ? F0[col - dcol] : 0.0; a1[k] = (dg && o1) ? F1[col - dcol] : 0.0;
    }
    (void)bw;
    for (int p = 0; p < nx; ++p) {
        const double e0 = E0[p], e1 = E1[p];
#pragma unroll
        for (int k = 0; k < TV_KC; ++k) {
            if (64 * k >= W) break;
            const int col = lane + 64 * k;
            const double x = col < W ? X[(size_t)p * ld + col] : 0.0;
            a0[k] += e0 * x; a1[k] += e1 * x;
        }
    }
    for (int q = 0; q < ny; ++q) {
        const double g0 = G0[q], g1 = G1[q];
#pragma unroll
        for (int k = 0; k < TV_KC; ++k) {
            if (64 * k >= W) break;
            const int col = lane + 64 * k;
            const double x = col < W ? Lr[(size_t)q * ld + col] : 0.0;
            a0[k] += g0 * x; a1[k] += g1 * x;
        }
    }
#pragma unroll
    for (int k = 0; k < TV_KC; ++k) {
        if (64 * k >= W) break;
        const int col = lane + 64 * k;
        if (col < W) { o0[col] = sign * a0[k]; if (o1) o1[col] = sign * a1[k]; }
    }
    for (int col = W + lane; col < full; col += 64) { o0[col] = 0.0; if (o1) o1[col] = 0.0; }
}

template <int TV_NX, int TV_KC, int TV_WPE>
__global__ void __launch_bounds__(512, TV_WPE) k_tv_rows(CondLayout L, CondPtrs P, const double *Qbuf, const double *S5buf)
{
    extern __shared__ double sm[];
    const int N = L.N, set = blockIdx.x, i = N - 1 - (int)blockIdx.y, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nwv = nt >> 6;
    const int nx = L.nx, nv = L.nv, nw = L.nw, ny = L.ny, nc = L.nc, nn = nx * nx;
    const int n = N * nv, nW = N * nw, W = (i + 1) * nv, Ww = (i + 1) * nw;
    const double *gset = P.pack + (size_t)set * N * P.pack_len;
    {
        const double *g = gset + (size_t)i * P.pack_len;
        const int tot = (int)P.pack_len;
#pragma unroll 8
        for (int e = tid; e < tot; e += nt) sm[e] = g[e];
    }
    double *stage = sm;
    auto take = [&](int len) -> double * { double *r = stage; stage += len; return r; };
    take(nn); take(nx * nw); take(nx);
    const double *C = take(ny * nx), *D4 = take(ny * nw), *d5 = take(ny), *E = take(nc * nx), *F4 = take(nc * nw), *f5 = take(nc),
                 *G = take(nc * ny);
    const int oB4 = nn, oBv = (int)(stage - sm);
    take(nx * nv);
    const double *Dv = take(ny * nv), *Fv = take(nc * nv);
    double *Qs = take(N * nn), *X = take(nx * n), *Xw = take(nx * nW), *Lv = take(ny * n), *Lw = take(ny * nW), *s5 = take(nx), *l5 = take(ny),
           *Lx = take(ny * nx);
    {
        const double *q = Qbuf + ((size_t)set * tv_tri(N) + tv_tri(i)) * nn;          // Q(i, -1 .. i-1): contiguous
        for (int e = tid; e < (i + 1) * nn; e += nt) Qs[e] = q[e];
        for (int e = tid; e < nx; e += nt) s5[e] = S5buf[((size_t)set * N + i) * nx + e];
    }
    double b0[TV_NX], b1[TV_NX];
#pragma unroll
    for (int rnd = 0; rnd < 2; ++rnd) {
        const int it = rnd * nt + tid;
        const bool live = it < W + Ww, isw = it >= W;
        const int col = isw ? it - W : it, bw = isw ? nw : nv, j = live ? col / bw : 0;
        const double *B = gset + (size_t)j * P.pack_len + (isw ? oB4 : oBv) + (col - j * bw);
#pragma unroll
        for (int p = 0; p < TV_NX; ++p) { const double v = (live && p < nx && j < i) ? B[p * bw] : 0.0; if (rnd == 0) b0[p] = v; else b1[p] = v; }
    }
    __syncthreads();
    // state family: X(:, block j) = Q(i,j) [B1 B2 B3 0]_j , zero on the diagonal block (step i's inputs act on x(i+1))
    // (a thread owns one column of one block, v and w columns in one index space: the nx loads of its column of B_j were issued
    //  before the barrier above, together with the staging loads -- one latency for everything this workgroup reads)
    for (int rnd = 0; rnd * nt < W + Ww; ++rnd) {
        const int it = rnd * nt + tid;
        if (it >= W + Ww) break;
        const bool isw = it >= W;
        const int col = isw ? it - W : it, bw = isw ? nw : nv, j = col / bw;
        double b[TV_NX], a[TV_NX];
        if (rnd < 2) {
#pragma unroll
            for (int p = 0; p < TV_NX; ++p) b[p] = rnd == 0 ? b0[p] : b1[p];
        } else {
            const double *B = gset + (size_t)j * P.pack_len + (isw ? oB4 : oBv) + (col - j * bw);
#pragma unroll
            for (int p = 0; p < TV_NX; ++p) b[p] = (p < nx && j < i) ? B[p * bw] : 0.0;
        }
#pragma unroll
        for (int p = 0; p < TV_NX; ++p) a[p] = 0.0;
        if (j < i) {
            const double *Q = Qs + (size_t)(j + 1) * nn;
#pragma unroll
            for (int p = 0; p < TV_NX; ++p) {
                if (p >= nx) break;
#pragma unroll
                for (int r = 0; r < TV_NX; ++r) { if (r >= nx) break; a[r] += Q[r * nx + p] * b[p]; }
            }
        }
        double *dst = isw ? Xw + col : X + col;
        const int ldx = isw ? nW : n;
#pragma unroll
        for (int r = 0; r < TV_NX; ++r) { if (r >= nx) break; dst[(size_t)r * ldx] = a[r]; }
    }
    for (int e = tid; e < ny * nx; e += nt) { const int r = e / nx, c = e - r * nx; double a = 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) a += C[r * nx + p] * Qs[p * nx + c]; Lx[e] = a; }
    for (int e = tid; e < ny; e += nt) { double a = 0.0; COND_UNROLL for (int p = 0; p < nx; ++p) a += C[e * nx + p] * s5[p]; l5[e] = a + d5[e]; }
    __syncthreads();
    // output family: L = C X + D on the diagonal block
    for (int e = tid; e < ny * W; e += nt) {
        const int r = e / W, col = e - r * W;
        double a = col >= i * nv ? Dv[r * nv + col - i * nv] : 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += C[r * nx + p] * X[(size_t)p * n + col];
        Lv[(size_t)r * n + col] = a;
    }
    for (int e = tid; e < ny * Ww; e += nt) {
        const int r = e / Ww, col = e - r * Ww;
        double a = col >= i * nw ? D4[r * nw + col - i * nw] : 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += C[r * nx + p] * Xw[(size_t)p * nW + col];
        Lw[(size_t)r * nW + col] = a;
    }
    __syncthreads();
    // whole output rows, one wave each (constraint rows in pairs), heaviest first
    double *oV[3], *oW[3], *oX[3], *o5[3];
    for (int f = 0; f < 3; ++f) {
        oV[f] = P.out[f * 4 + 1] ? P.out[f * 4 + 1] + (size_t)set * L.out_size[f * 4 + 1] + (size_t)i * L.rows[f] * n : nullptr;
        oW[f] = P.out[f * 4 + 2] ? P.out[f * 4 + 2] + (size_t)set * L.out_size[f * 4 + 2] + (size_t)i * L.rows[f] * nW : nullptr;
        oX[f] = P.out[f * 4 + 0] ? P.out[f * 4 + 0] + (size_t)set * L.out_size[f * 4 + 0] + (size_t)i * L.rows[f] * nx : nullptr;
        o5[f] = P.out[f * 4 + 3] ? P.out[f * 4 + 3] + (size_t)set * L.out_size[f * 4 + 3] + (size_t)i * L.rows[f] : nullptr;
    }
    const int hp = (nc + 1) / 2;
    const int t_hv = oV[2] ? hp : 0, t_hw = oW[2] ? hp : 0, t_gv = oV[0] ? nx : 0, t_lv = oV[1] ? ny : 0, t_gw = oW[0] ? nx : 0, t_lw = oW[1] ? ny : 0;
    const int ntask = t_hv + t_hw + t_gv + t_lv + t_gw + t_lw;
    for (int t = wave; t < ntask; t += nwv) {
        int u = t;
        if (u < t_hv) {
            const int r0 = 2 * u, r1 = r0 + 1 < nc ? r0 + 1 : r0;
            tv_hrows<TV_KC>(oV[2] + (size_t)r0 * n, r0 + 1 < nc ? oV[2] + (size_t)r1 * n : nullptr, E + r0 * nx, E + r1 * nx, G + r0 * ny, G + r1 * ny,
                     Fv + r0 * nv, Fv + r1 * nv, X, Lv, nx, ny, n, W, n, i * nv, nv, 1.0, lane);
            continue;
        }
        u -= t_hv;
        if (u < t_hw) {
            const int r0 = 2 * u, r1 = r0 + 1 < nc ? r0 + 1 : r0;
            tv_hrows<TV_KC>(oW[2] + (size_t)r0 * nW, r0 + 1 < nc ? oW[2] + (size_t)r1 * nW : nullptr, E + r0 * nx, E + r1 * nx, G + r0 * ny, G + r1 * ny,
                     F4 + r0 * nw, F4 + r1 * nw, Xw, Lw, nx, ny, nW, Ww, nW, i * nw, nw, -1.0, lane);
            continue;
        }
        u -= t_hw;
        const double *src; double *dst; int wid, full;
        if (u < t_gv) { src = X + (size_t)u * n; dst = oV[0] + (size_t)u * n; wid = W; full = n; }
        else if ((u -= t_gv) < t_lv) { src = Lv + (size_t)u * n; dst = oV[1] + (size_t)u * n; wid = W; full = n; }
        else if ((u -= t_lv) < t_gw) { src = Xw + (size_t)u * nW; dst = oW[0] + (size_t)u * nW; wid = Ww; full = nW; }
        else { u -= t_gw; src = Lw + (size_t)u * nW; dst = oW[1] + (size_t)u * nW; wid = Ww; full = nW; }
        for (int col = lane; col < full; col += 64) dst[col] = col < wid ? src[col] : 0.0;
    }
    // x / constant columns of block-row i: Qs[0] = A_{i-1} ... A_0, s5 = sum_j A_{i-1} ... A_{j+1} b5_j
    if (oX[0]) for (int e = tid; e < nn; e += nt) oX[0][e] = Qs[e];
    if (o5[0]) for (int e = tid; e < nx; e += nt) o5[0][e] = s5[e];
    if (oX[1]) for (int e = tid; e < ny * nx; e += nt) oX[1][e] = Lx[e];
    if (o5[1]) for (int e = tid; e < ny; e += nt) o5[1][e] = l5[e];
    if (oX[2]) for (int e = tid; e < nc * nx; e += nt) {
        const int r = e / nx, c = e - r * nx;
        double a = 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += E[r * nx + p] * Qs[p * nx + c];
        COND_UNROLL for (int p = 0; p < ny; ++p) a += G[r * ny + p] * Lx[p * nx + c];
        oX[2][e] = -a;
    }
    if (o5[2]) for (int e = tid; e < nc; e += nt) {
        double a = 0.0;
        COND_UNROLL for (int p = 0; p < nx; ++p) a += E[e * nx + p] * s5[p];
        COND_UNROLL for (int p = 0; p < ny; ++p) a += G[e * ny + p] * l5[p];
        o5[2][e] = f5[e] - a;
    }
}

static size_t condense_tv_rows_lds(const CondLayout &L, size_t pack_len)
{
    const size_t N = L.N;
    return sizeof(double) * (pack_len + N * L.nx * L.nx + (size_t)(L.nx + L.ny) * N * (L.nv + L.nw) + L.nx + L.ny + (size_t)L.ny * L.nx + 16);
}

static size_t condense_tv_lds(const CondLayout &L, size_t pack_len)
{
    return sizeof(double) * (pack_len + (size_t)3 * L.nx * L.nx + (size_t)(1 + COND_TV_JB) * L.nx * (L.nv + L.nw) + 3 * (size_t)L.nx +
                             (size_t)COND_TV_JB * L.ny * (L.nv + L.nw) + (size_t)L.ny * L.nx + L.ny + 16);
}

int condense_model_device(mld_model *m, int N, double *kernel_ms, hipStream_t stream, bool f32)
{
    if (f32 && m->tv_N > 0) { mld_set_error("fp32 materialisation is implemented for time-invariant models only"); return MLD_ERR_UNSUPPORTED; }
    if (N < 1) { mld_set_error("N_tilde must be >= 1"); return MLD_ERR_INVALID; }
    if (m->tv_N > 0 && N != m->tv_N) { mld_set_error("time-varying model holds %d step models per horizon, N_tilde = %d asked", m->tv_N, N); return MLD_ERR_INVALID; }
    if (m->cond_N != N) {
        m->d_blocks.reset();
        for (int k = 0; k < 12; ++k) { m->d_out[k].reset(); m->d_out32[k].reset(); }
        m->d_tvQ.reset(); m->d_tvS.reset();
        compute_layout(m->dims, N, &m->lay);
        HIP_TRY(m->d_blocks.alloc(m->lay.blk_stride * m->n_models));
        for (int k = 0; k < 12; ++k)
            if (m->lay.out_size[k]) HIP_TRY(m->d_out[k].alloc(m->lay.out_size[k] * m->n_models));
        m->cond_N = N; m->out64 = false;
    }
    if (f32) for (int k = 0; k < 12; ++k) if (m->lay.out_size[k] && !m->d_out32[k]) HIP_TRY(m->d_out32[k].alloc(m->lay.out_size[k] * m->n_models));
    CondPtrs P;
    for (int k = 0; k < 20; ++k) { P.mats[k] = m->d_mats[k]; P.mat_size[k] = m->mat_size[k]; }
    P.blocks = m->d_blocks;
    for (int k = 0; k < 12; ++k) P.out[k] = m->d_out[k];
    P.pack = m->d_pack; P.pack_len = m->pack_len;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    if (m->tv_N > 0) {   // one model per horizon step: block-rows computed and written in one pass
        const size_t lds_rows = condense_tv_rows_lds(m->lay, m->pack_len);
        const size_t nn = (size_t)m->lay.nx * m->lay.nx;
        const size_t lds_chain = sizeof(double) * ((size_t)N * nn + (size_t)N * m->lay.nx + 16 * 2 * nn + 16);   // k_tv_chain: all A_i, b5_i + 16 waves x 2 nx^2
        const int wmax = N * (m->lay.nv > m->lay.nw ? m->lay.nv : m->lay.nw);
        const bool small = wmax <= 640 && m->lay.nx <= 8;                      // <8, 10>: row accumulators and B columns in fewer registers
        const bool wide = m->pack_len && lds_rows <= 144 * 1024 && lds_chain <= 160 * 1024 && wmax <= 1024 && m->lay.nx <= 16 && !(getenv("MLD_TV_CHAIN_ONLY"));
        if (wide) {
            const CondLayout &L = m->lay;
            const size_t qlen = (size_t)m->n_models * (N * (N + 1) / 2) * nn, slen = (size_t)m->n_models * N * L.nx;
            if (!m->d_tvQ) { HIP_TRY(m->d_tvQ.alloc(qlen)); HIP_TRY(m->d_tvS.alloc(slen)); }
            if (lds_chain > 48 * 1024) (void)hipFuncSetAttribute((const void *)k_tv_chain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_chain);
            void (*rows)(CondLayout, CondPtrs, const double *, const double *) = small ? k_tv_rows<8, 10, 4> : k_tv_rows<16, 16, 2>;
            if (lds_rows > 48 * 1024) (void)hipFuncSetAttribute((const void *)rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows);
            HIP_TRY(hipEventRecord(e0, stream));
            hipLaunchKernelGGL(k_tv_chain, dim3(m->n_models), dim3(1024), lds_chain, stream, m->lay, P, m->d_tvQ, m->d_tvS);
            hipLaunchKernelGGL(rows, dim3(m->n_models, N), dim3(512), lds_rows, stream, m->lay, P, (const double *)m->d_tvQ, (const double *)m->d_tvS);
            HIP_TRY(hipEventRecord(e1, stream));
            HIP_TRY(hipEventSynchronize(e1));
            HIP_TRY(hipGetLastError());
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
            if (kernel_ms) *kernel_ms = ms;
            (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
            m->out64 = true;
            return MLD_OK;
        }
        const size_t lds = condense_tv_lds(m->lay, m->pack_len);
        if (lds > 150 * 1024) { mld_set_error("time-varying condensing: step model too large for LDS (%zu bytes)", lds); return MLD_ERR_UNSUPPORTED; }
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)k_condense_tv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        HIP_TRY(hipEventRecord(e0, stream));
        if (m->pack_len) hipLaunchKernelGGL(k_condense_tv, dim3(m->n_models, N), dim3(256), lds, stream, m->lay, P);
        HIP_TRY(hipEventRecord(e1, stream));
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipGetLastError());
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        if (kernel_ms) *kernel_ms = ms;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        m->out64 = true;
        return MLD_OK;
    }
    HIP_TRY(hipEventRecord(e0, stream));
    {
        const CondLayout &L = m->lay;
        const size_t lds = sizeof(double) * ((size_t)3 * L.nx * L.nx + 2 * L.nx + (size_t)(2 * L.nx + 2 * L.ny + L.nc) * L.nv +
                                            (size_t)(L.nx + L.ny) * L.nw + (size_t)L.ny * L.nx + L.ny + 16 +
                                            (size_t)L.nx * L.nx + (size_t)(L.nx + L.ny + L.nc) * L.nw + L.nx + (size_t)L.ny * L.nx + L.ny +
                                            (size_t)L.nc * L.nx + L.nc + (size_t)L.nc * L.ny);
        // blocks of one model are dealt to `split` workgroups (each repeats the cheap prefix doubling) until the grid fills the chip
        int split = 1;
        while (split < N && (size_t)m->n_models * split < 512) split *= 2;
        if (split > N) split = N;
        if (getenv("MLD_K1_SPLIT")) split = atoi(getenv("MLD_K1_SPLIT"));
        if (split < 1) split = 1;
        const size_t lds_model = condense_model_lds(L, m->pack_len, split);
        const int threads = split >= 4 ? 256 : (split == 2 ? 512 : 1024);
        if (m->pack_len && lds_model <= 144 * 1024 && !getenv("MLD_K1_PER_BLOCK")) {
            if (lds_model > 48 * 1024) (void)hipFuncSetAttribute((const void *)k_condense_model, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_model);
            hipLaunchKernelGGL(k_condense_model, dim3(m->n_models, split), dim3(threads), lds_model, stream, m->lay, P);
        } else
            hipLaunchKernelGGL(k_condense_blocks, dim3(N, m->n_models), dim3(128), lds, stream, m->lay, P);
    }
    const int rows_total = N * (m->dims.nx + m->dims.ny + m->dims.nc);
    if (rows_total > 0) {
        FlatJobs J; J.n = 0;
        unsigned nblk = 0; bool flat_ok = true;
        for (int f = 0; f < 3 && flat_ok; ++f)
            for (int w2 = 0; w2 < 4; ++w2) {
                const int k = f * 4 + (w2 == 0 ? 1 : (w2 == 1 ? 2 : (w2 == 2 ? 0 : 3)));     /* out order: x, v, w, 5 */
                const int bw = w2 == 0 ? m->lay.nv : (w2 == 1 ? m->lay.nw : (w2 == 2 ? m->lay.nx : 1));
                if (!m->d_out[k] || !m->lay.out_size[k] || !bw) continue;
                const size_t tot = m->lay.out_size[k] * (size_t)m->n_models;
                if (tot >= 0xfffff000ull) { flat_ok = false; break; }          /* 32-bit flat indices */
                FlatJob &jb = J.j[J.n++];
                jb.out = f32 ? (void *)m->d_out32[k] : (void *)m->d_out[k]; jb.blk_off_dummy = nullptr; jb.total = (unsigned)tot; jb.per_model = (unsigned)m->lay.out_size[k];
                jb.rows = N * m->lay.rows[f]; jb.width = w2 < 2 ? N * bw : bw; jb.bw = bw; jb.fam = f; jb.is_w = w2; jb.first_block = nblk;
                { const size_t chunk = f32 ? 2 * (size_t)COND_FLAT : (size_t)COND_FLAT; nblk += (unsigned)((tot + chunk - 1) / chunk); }
            }
        if (flat_ok && J.n > 0 && f32) hipLaunchKernelGGL(k_condense_flat<float>, dim3(nblk), dim3(256), 0, stream, m->lay, P, J);
        else if (flat_ok && J.n > 0) hipLaunchKernelGGL(k_condense_flat<double>, dim3(nblk), dim3(256), 0, stream, m->lay, P, J);
        else if (f32) { mld_set_error("fp32 materialisation: output too large for 32-bit flat indices"); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return MLD_ERR_UNSUPPORTED; }
        else hipLaunchKernelGGL(k_condense_scatter, dim3((rows_total + COND_ROWS_PER_WG - 1) / COND_ROWS_PER_WG, m->n_models), dim3(256), 0, stream, m->lay, P, rows_total, 0);
    }
    HIP_TRY(hipEventRecord(e1, stream));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipGetLastError());
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (kernel_ms) *kernel_ms = ms;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (!f32) m->out64 = true;
    return MLD_OK;
}
