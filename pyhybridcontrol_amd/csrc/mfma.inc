// The instance-GEMM core: a batch's per-instance vectors times a model's matrix, as ONE batched GEMM per model with the batch as
// the M dimension.  A workgroup owns up to RM_NI instances of ONE model (a RhsGroup), keeps their vectors in registers as MFMA
// A fragments (instances along M), and streams the model's matrix through an LDS tile sixteen rows (or columns) at a time as the
// B operand, so the matrix is read once per RM_NI instances and the output is written as 128-byte segments.  An inner dimension
// that does not fit the registers goes in chunks of IG_KC with the output as the accumulator.  v_mfma_f64_16x16x4_f64 (fp64)
// or v_mfma_f32_16x16x4_f32 (MLD_F32: inputs rounded to fp32, fp32 accumulate).
// Lane maps (guides/cdna_hip_programming.md): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15];
// f64 C/D: col = l & 15, row = (l >> 4) + 4 r;  f32 C/D: col = l & 15, row = 4 (l >> 4) + r.
// The pieces (all inlined; li = lane & 15, lk = lane >> 4): ig_slots (a lane's instances), ig_load_a (A fragments), ig_stage
// (sixteen rows into an LDS tile), ig_mma (the MFMA chain), ig_bits (masks of groups of four inner indices).  The members
// -- k_rhs_mfma below, k_inst_pullback (inst_cost.inc), k_trajectory (trajectory.inc), k_evaluate (evaluate.inc) -- add what
// they read, the groups they may skip, and their epilogue.
#pragma once

#define RM_WAVES 8
#define RM_NI (16 * RM_WAVES)        // instances per workgroup
#define RM_KMAX 320                  // K = nx + N nw padded to a multiple of 4 (cfg3: 208); larger shapes use k_rhs
#define RM_KS (RM_KMAX / 4)
#define IG_KC 256                    // inner-dimension chunk (of the chunked members) whose A fragments live in registers
#define IG_KS (IG_KC / 4)
#define IG_LD (IG_KC + 1)            // row stride of a staged [16][IG_KC] tile (odd: few bank conflicts)

typedef double rm_f64x4 __attribute__((ext_vector_type(4)));
typedef float rm_f32x4 __attribute__((ext_vector_type(4)));

struct RhsGroup { int model, start, count; };    // instances perm[start .. start + count) share `model`

template <bool F32, int KS> struct IgFrag { double a64[F32 ? 1 : KS]; float a32[F32 ? KS : 1]; };      // A fragments of KS groups of four

// the instance whose A fragments this lane holds (the return value) and the instances of its four C/D rows; -1 past the group's end
template <bool F32>
__device__ __forceinline__ int ig_slots(const RhsGroup &g, const int *perm, int wave, int li, int lk, int (&oinst)[4])
{
    auto at = [=](int slot) { return slot < g.count ? (perm ? perm[g.start + slot] : g.start + slot) : -1; };
    const int inst = at(wave * 16 + li);
#pragma unroll
    for (int r = 0; r < 4; ++r) oinst[r] = at(wave * 16 + (F32 ? 4 * lk + r : lk + 4 * r));
    return inst;
}

// A fragments of the chunk that begins at kc0 and has ks groups: a[s] = load(k), k = kc0 + 4 s + lk < K; zero past K and in a lane without
// an instance.  (The loaders and predicates capture by value: what a lambda reaches through a reference the compiler may leave in memory.)
template <bool F32, int KS, typename Load>
__device__ __forceinline__ void ig_load_a(IgFrag<F32, KS> &a, int inst, int kc0, int lk, int ks, int K, Load load)
{
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        double v = 0.0;
        const int k = kc0 + 4 * s + lk;
        if (s < ks && inst >= 0 && k < K) v = load(k);
        if (F32) a.a32[s] = (float)v; else a.a64[s] = v;
    }
}

// bits lo .. hi - 1 of a chunk's mask of groups of four inner indices (clipped to the IG_KS groups of a chunk)
static_assert(IG_KS == 64, "a chunk's groups of four are one 64-bit mask");
__device__ __forceinline__ unsigned long long ig_bits(int lo, int hi)
{
    lo = max(lo, 0); hi = min(hi, IG_KS);
    if (hi <= lo) return 0ull;
    return (hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1ull) << lo;
}
struct IgMask {                      // such a mask as ig_mma's predicate
    unsigned long long need;
    __device__ bool operator()(int s) const { return (need >> s & 1ull) != 0; }
};

// tile[i][kk] = at(rb + i, kc0 + kk) for sixteen rows and the groups of four in `need`, coalesced along each row, between two barriers;
// skipped groups are neither read nor written
template <typename At>
__device__ __forceinline__ void ig_stage(double *tile, int tid, int rb, int kc0, unsigned long long need, At at)
{
    __syncthreads();
    for (int e = tid; e < 16 * IG_KC; e += 64 * RM_WAVES) {
        const int i = e / IG_KC, kk = e % IG_KC;
        if (need >> (kk >> 2) & 1ull) tile[i * IG_LD + kk] = at(rb + i, kc0 + kk);
    }
    __syncthreads();
}

// res[r] = sum over the groups s with use(s) of A[.][4 s ..] B[4 s ..][li], B[k = 4 s + lk][j = li] = brow[STRIDE * s].  Two accumulators
// hide the dependent latency of the chain: even s into one, odd s into the other, summed at the end (in float under F32, then widened).
template <int STRIDE, bool F32, int KS, typename Use>
__device__ __forceinline__ void ig_mma(const IgFrag<F32, KS> &a, const double *brow, Use use, double (&res)[4])
{
    if (F32) {
        rm_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; s += 2) {
            if (use(s)) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.a32[s], (float)brow[STRIDE * s], acc0, 0, 0, 0);
            if (use(s + 1)) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.a32[s + 1], (float)brow[STRIDE * (s + 1)], acc1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) res[r] = (double)(acc0[r] + acc1[r]);
    } else {
        rm_f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < KS; s += 2) {
            if (use(s)) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.a64[s], brow[STRIDE * s], acc0, 0, 0, 0);
            if (use(s + 1)) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.a64[s + 1], brow[STRIDE * (s + 1)], acc1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) res[r] = acc0[r] + acc1[r];
    }
}

// K3, the constraint right-hand sides of a whole batch:
//     hs[b, :] = rs .* ([H_x | H_w] [x0_b ; w_b] + H_5)          (controllers/controller_base.py:446-450)
// (SURVEY section 2, kernel K3: "[500 x 207] . [207 x B]").  k_rhs re-streams a model's 0.83 MB of H for every instance (measured
// 13-26x over-fetch).  What it adds to the core: no chunks -- all K <= RM_KMAX of [x0 ; w] in registers, a dynamic tile of all Kp
// columns -- and the epilogue with H_5 and the row scale.
template <bool F32>
__global__ void __launch_bounds__(64 * RM_WAVES) k_rhs_mfma(int m0, int nx, int nW, int Kp, const double *Hx, const double *Hw, const double *H5,
                                                            const double *rs, const RhsGroup *groups, const int *perm, const double *x0,
                                                            const double *omega, double *hs)
{
    extern __shared__ double rm_tile[];              // 16 rows x (Kp + 1) doubles of [H_x | H_w] (odd stride: few bank conflicts)
    const RhsGroup g = groups[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int ld = Kp + 1, K = nx + nW, ks = Kp >> 2;
    const double *hx = Hx ? Hx + (size_t)g.model * m0 * nx : nullptr, *hw = Hw ? Hw + (size_t)g.model * m0 * nW : nullptr;
    const double *h5 = H5 + (size_t)g.model * m0, *rsm = rs ? rs + (size_t)g.model * m0 : nullptr;
    int oinst[4];
    const int inst = ig_slots<F32>(g, perm, wave, li, lk, oinst);
    IgFrag<F32, RM_KS> a;
    ig_load_a(a, inst, 0, lk, ks, K, [=](int k) { return k < nx ? x0[(size_t)inst * nx + k] : omega[(size_t)inst * nW + (k - nx)]; });
    for (int rb = 0; rb < m0; rb += 16) {
        __syncthreads();
        // stage rows rb .. rb+15 of [H_x | H_w] (zero padded), coalesced along each row
        for (int e = tid; e < 16 * Kp; e += 64 * RM_WAVES) {
            const int i = e / Kp, k = e - i * Kp, row = rb + i;
            double v = 0.0;
            if (row < m0 && k < K) v = k < nx ? (hx ? hx[(size_t)row * nx + k] : 0.0) : (hw ? hw[(size_t)row * nW + (k - nx)] : 0.0);
            rm_tile[i * ld + k] = v;
        }
        __syncthreads();
        const int row = rb + li;
        double res[4];
        ig_mma<4>(a, rm_tile + li * ld + lk, [ks](int s) { return s < ks; }, res);          // B = H[rb + li][k]
        if (row < m0) {
            const double c5 = h5[row], sc = rsm ? rsm[row] : 1.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) if (oinst[r] >= 0) hs[(size_t)oinst[r] * m0 + row] = (res[r] + c5) * sc;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K4 on the matrix cores: C (M x Nn) = alpha op(A) B + beta C, batched over models (blockIdx.z), fp64 MFMA 16x16x4 (or fp32 with
// MLD_F32).  The quadratic cost pull-back  P += Gamma' (W + W') Gamma  (controllers/components/objective_atoms.py:321-331 through
// variables.py:259-275) is two such products with inner dimension N_tilde * nx (cfg3: 175).  A workgroup of 4 waves owns a
// 64 x 64 tile of C; K is staged through LDS 16 at a time (A tile 64 x 16 as [row][k], B tile 16 x 64 as [k][col], padded
// strides); a wave owns 16 rows x 64 columns = four accumulator tiles, so every A fragment feeds four MFMAs.
#define GM_T 64
#define GM_K 16
template <bool F32>
__global__ void __launch_bounds__(256) k_gemm_mfma(int M, int Nn, int K, int transA, const double *A, size_t sA, const double *Bm, size_t sB,
                                                  double *Cm, size_t sC, double alpha, double beta)
{
    __shared__ double tA[GM_T][GM_K + 1], tB[GM_K][GM_T + 1];
    const int mdl = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const double *a = A + (size_t)mdl * sA, *b = Bm + (size_t)mdl * sB;
    double *c = Cm + (size_t)mdl * sC;
    const int row0 = blockIdx.y * GM_T, col0 = blockIdx.x * GM_T;
    rm_f64x4 acc[4]; rm_f32x4 accf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { acc[t] = (rm_f64x4){0.0, 0.0, 0.0, 0.0}; accf[t] = (rm_f32x4){0.f, 0.f, 0.f, 0.f}; }
    for (int k0 = 0; k0 < K; k0 += GM_K) {
        __syncthreads();
        for (int e = tid; e < GM_T * GM_K; e += 256) {
            // A tile: coalesced along the contiguous dimension of the stored matrix (k when not transposed, row when transposed)
            const int i = transA ? e % GM_T : e / GM_K, k = transA ? e / GM_T : e % GM_K;
            const int row = row0 + i, kk = k0 + k;
            tA[i][k] = (row < M && kk < K) ? (transA ? a[(size_t)kk * M + row] : a[(size_t)row * K + kk]) : 0.0;
            const int kb = e / GM_T, j = e % GM_T, col = col0 + j;
            tB[kb][j] = (k0 + kb < K && col < Nn) ? b[(size_t)(k0 + kb) * Nn + col] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GM_K; kk += 4) {
            const double av = tA[wave * 16 + li][kk + lk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double bv = tB[kk + lk][t * 16 + li];
                if (F32) accf[t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)av, (float)bv, accf[t], 0, 0, 0);
                else acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + wave * 16 + (F32 ? 4 * lk + r : lk + 4 * r), col = col0 + t * 16 + li;
            if (row < M && col < Nn) {
                const double v = F32 ? (double)accf[t][r] : acc[t][r];
                double *dst = c + (size_t)row * Nn + col;
                *dst = alpha * v + (beta != 0.0 ? beta * *dst : 0.0);
            }
        }
}
