// Host side of the problem handle: big-M tightening (per model, once), scaling, cost pull-back (K4),
// workspace management, batch upload / solve / download, RCCL gather.
#include <rccl/rccl.h>

#include "mfma.inc"
#include "inst_cost.inc"
#include "lp_lds.inc"

#include <limits>
#include <memory>

// ------------------------------------------------------------------------------------------------
// probing-based coefficient tightening of one step's MLD rows (Savelsbergh 1994, sections 1.1, 3.2-3.3).
// MLD models are big-M translations of logic; with loose constants the LP relaxation of the condensed
// problem is very weak.  Integer-feasible points are unchanged.  Works on W = [E F1 F2 F3 F4 G Psi].
// ------------------------------------------------------------------------------------------------
namespace tighten {
static const double INF = std::numeric_limits<double>::infinity();

static bool propagate(const std::vector<double> &W, const std::vector<double> &c, int nc, int nt, std::vector<double> &lb,
                      std::vector<double> &ub, const std::vector<char> &is_int)
{
    for (int pass = 0; pass < 6; ++pass) {
        bool changed = false;
        for (int i = 0; i < nc; ++i) {
            const double *a = &W[(size_t)i * nt];
            double tot = 0; int ninf = 0, jinf = -1, nnz = 0;
            for (int j = 0; j < nt; ++j) {
                if (a[j] == 0) continue;
                nnz++;
                const double lc = a[j] > 0 ? a[j] * lb[j] : a[j] * ub[j];
                if (std::isinf(lc)) { ninf++; jinf = j; } else tot += lc;
            }
            if (!nnz) continue;
            if (!ninf && tot > c[i] + 1e-9 * std::max(1.0, std::fabs(c[i]))) return false;
            if (ninf > 1) continue;
            for (int j = 0; j < nt; ++j) {
                if (a[j] == 0) continue;
                double rest;
                if (!ninf) rest = tot - (a[j] > 0 ? a[j] * lb[j] : a[j] * ub[j]);
                else if (j == jinf) rest = tot;
                else continue;
                double b = (c[i] - rest) / a[j];
                if (a[j] > 0) {
                    if (is_int[j]) b = std::floor(b + 1e-9);
                    if (b < ub[j] - 1e-12 * std::max(1.0, std::fabs(b))) { ub[j] = b; changed = true; }
                } else {
                    if (is_int[j]) b = std::ceil(b - 1e-9);
                    if (b > lb[j] + 1e-12 * std::max(1.0, std::fabs(b))) { lb[j] = b; changed = true; }
                }
            }
        }
        for (int j = 0; j < nt; ++j) if (lb[j] > ub[j] + 1e-9) return false;
        if (!changed) break;
    }
    return true;
}

static double max_activity(const double *a, int nt, const std::vector<double> &lb, const std::vector<double> &ub, int skip)
{
    double s = 0;
    for (int j = 0; j < nt; ++j) {
        if (j == skip || a[j] == 0) continue;
        s += a[j] > 0 ? a[j] * ub[j] : a[j] * lb[j];
    }
    return s;
}

// mats: 20 host matrices of ONE model (row-major); modifies E..Psi / f5 copies in place
static void run(const mld_dims &d, std::vector<std::vector<double>> &mats, size_t model, int rounds = 2)
{
    const int sizes[7] = {d.nx, d.nu, d.ndelta, d.nz, d.nomega, d.ny, d.nmu};
    const int ids[7] = {MT_E, MT_F1, MT_F2, MT_F3, MT_F4, MT_G, MT_Psi};
    int offs[8]; offs[0] = 0;
    for (int k = 0; k < 7; ++k) offs[k + 1] = offs[k] + sizes[k];
    const int nt = offs[7], nc = d.nc;
    if (!nc || !nt) return;
    std::vector<double> W((size_t)nc * nt, 0.0), c(nc, 0.0);
    for (int k = 0; k < 7; ++k)
        for (int i = 0; i < nc; ++i)
            for (int j = 0; j < sizes[k]; ++j)
                W[(size_t)i * nt + offs[k] + j] = mats[ids[k]][model * (size_t)nc * sizes[k] + (size_t)i * sizes[k] + j];
    for (int i = 0; i < nc; ++i) c[i] = mats[MT_f5][model * (size_t)nc + i];
    std::vector<double> lb(nt, -INF), ub(nt, INF);
    std::vector<char> is_int(nt, 0);
    std::vector<int> bins;
    for (int j = offs[1] + d.nu - d.nu_l; j < offs[1] + d.nu; ++j) bins.push_back(j);
    for (int j = offs[2]; j < offs[2] + d.ndelta; ++j) bins.push_back(j);
    for (int j = offs[6] + d.nmu - d.nmu_l; j < offs[6] + d.nmu; ++j) bins.push_back(j);
    for (int j = offs[6]; j < offs[6] + d.nmu; ++j) lb[j] = 0.0;          // mu >= 0 (variables.py:221)
    for (int j : bins) { lb[j] = 0; ub[j] = 1; is_int[j] = 1; }
    for (int rnd = 0; rnd < rounds; ++rnd) {
        if (!propagate(W, c, nc, nt, lb, ub, is_int)) return;           // rows infeasible on their own: leave alone
        const size_t nbn = bins.size();
        std::vector<std::vector<double>> cl(2 * nbn), cu(2 * nbn);
        std::vector<char> ok(2 * nbn, 0);
        for (size_t t = 0; t < nbn; ++t)
            for (int v = 0; v < 2; ++v) {
                const int b = bins[t];
                if (!(lb[b] <= v && v <= ub[b])) continue;
                cl[2 * t + v] = lb; cu[2 * t + v] = ub;
                cl[2 * t + v][b] = cu[2 * t + v][b] = v;
                ok[2 * t + v] = propagate(W, c, nc, nt, cl[2 * t + v], cu[2 * t + v], is_int);
            }
        for (size_t t = 0; t < nbn; ++t) {
            if (!ok[2 * t] && ok[2 * t + 1]) lb[bins[t]] = 1.0;
            else if (!ok[2 * t + 1] && ok[2 * t]) ub[bins[t]] = 0.0;
        }
        for (int i = 0; i < nc; ++i)
            for (size_t t = 0; t < nbn; ++t) {
                const int b = bins[t];
                double *a = &W[(size_t)i * nt];
                const double ab = a[b];
                if (ab == 0.0) continue;
                if (ab > 0) {                    // b = 0 side: rest <= c_i
                    if (!ok[2 * t]) continue;
                    const double U = max_activity(a, nt, cl[2 * t], cu[2 * t], b);
                    if (std::isfinite(U) && U < c[i] - 1e-12 * std::max(1.0, std::fabs(c[i]))) { const double dl = c[i] - U; c[i] = U; a[b] = ab - dl; }
                } else {                         // b = 1 side: rest <= c_i - a_b
                    if (!ok[2 * t + 1]) continue;
                    const double U = max_activity(a, nt, cl[2 * t + 1], cu[2 * t + 1], b);
                    if (std::isfinite(U) && U < c[i] - ab - 1e-12 * std::max(1.0, std::fabs(c[i] - ab))) a[b] = c[i] - U;
                }
            }
    }
    for (int k = 0; k < 7; ++k)
        for (int i = 0; i < nc; ++i)
            for (int j = 0; j < sizes[k]; ++j)
                mats[ids[k]][model * (size_t)nc * sizes[k] + (size_t)i * sizes[k] + j] = W[(size_t)i * nt + offs[k] + j];
    for (int i = 0; i < nc; ++i) mats[MT_f5][model * (size_t)nc + i] = c[i];
}
} // namespace tighten

// ------------------------------------------------------------------------------------------------
// K4 kernels: linear pull-back (one workgroup per model) and small dense GEMMs for the quadratic part
// ------------------------------------------------------------------------------------------------
// out[j] = base[j] + sum_i A[i, j] * w[i]      A is (rows x cols) row-major; threads own columns
__global__ void __launch_bounds__(256) k_pullback(int rows, int cols, const double *A, size_t strideA, const double *w,
                                                 size_t strideW, double *out, size_t strideO, int accumulate)
{
    const int mdl = blockIdx.y;
    const double *a = A + (size_t)mdl * strideA, *ww = w + (size_t)mdl * strideW;
    double *o = out + (size_t)mdl * strideO;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < cols; j += gridDim.x * blockDim.x) {
        double s = accumulate ? o[j] : 0.0;
        for (int i = 0; i < rows; ++i) s += a[(size_t)i * cols + j] * ww[i];
        o[j] = s;
    }
}

// C (M x Nn) = alpha * op(A) * B + beta * C ;  op(A) = A^T when transA (A stored K x M) ; batched over models
__global__ void __launch_bounds__(256) k_gemm(int M, int Nn, int K, int transA, const double *A, size_t sA, const double *Bm,
                                             size_t sB, double *Cm, size_t sC, double alpha, double beta)
{
    __shared__ double tA[16][17], tB[16][17];
    const int mdl = blockIdx.z;
    const double *a = A + (size_t)mdl * sA, *b = Bm + (size_t)mdl * sB;
    double *c = Cm + (size_t)mdl * sC;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int row = blockIdx.y * 16 + ty, col = blockIdx.x * 16 + tx;
    double acc = 0.0;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int ka = k0 + tx, kb = k0 + ty;
        tA[ty][tx] = (row < M && ka < K) ? (transA ? a[(size_t)ka * M + row] : a[(size_t)row * K + ka]) : 0.0;
        tB[ty][tx] = (kb < K && col < Nn) ? b[(size_t)kb * Nn + col] : 0.0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) acc += tA[ty][k] * tB[k][tx];
        __syncthreads();
    }
    if (row < M && col < Nn) c[(size_t)row * Nn + col] = alpha * acc + (beta != 0.0 ? beta * c[(size_t)row * Nn + col] : 0.0);
}

// out = W + W^T  (square, batched)
__global__ void k_symmetrize(int n, const double *W, double *out, size_t stride)
{
    const int mdl = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (size_t)n * n) { const size_t i = e / n, j = e % n; out[mdl * stride + e] = W[mdl * stride + e] + W[mdl * stride + j * n + i]; }
}


// qs_inst[b][j] = cs[j] * (q0[j] + Qx[j,:] x0_b + Qw[j,:] w_b)   (quadratic atoms on x / y make q depend on the parameters);
// qadd (batch x ldq, or null): the per-instance linear cost of mld_upload_instance_cost, added to q0
__global__ void __launch_bounds__(256) k_qinst(int n, int nx, int nW, const double *q0, const double *Qx, const double *Qw, const double *cs,
                                              const int *model_idx, const double *x0, const double *omega, double *qs_inst,
                                              const double *qadd, int ldq)
{
    const int b = blockIdx.x, mdl = model_idx ? model_idx[b] : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const double *xb = x0 + (size_t)b * nx, *wb = omega + (size_t)b * nW;
    for (int j = wave; j < n; j += nwv) {
        double acc = 0.0;
        if (Qx) { const double *r = Qx + ((size_t)mdl * n + j) * nx; for (int k = lane; k < nx; k += 64) acc += r[k] * xb[k]; }
        if (Qw) { const double *r = Qw + ((size_t)mdl * n + j) * nW; for (int k = lane; k < nW; k += 64) acc += r[k] * wb[k]; }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if (lane == 0) {
            const double base = qadd ? q0[(size_t)mdl * n + j] + qadd[(size_t)b * ldq + j] : q0[(size_t)mdl * n + j];
            qs_inst[(size_t)b * n + j] = (base + acc) * cs[(size_t)mdl * n + j];
        }
    }
}

// rconst[b] += e' W e with e = Mx x0_b + Mw w_b + m0  (value of a quadratic atom at v = 0); one workgroup per instance
__global__ void __launch_bounds__(256) k_quad_const(int len, int nx, int nW, const double *Mx, size_t sMx, const double *Mw, size_t sMw,
                                                   const double *m0, size_t sm0, const double *W, const int *model_idx,
                                                   const double *x0, const double *omega, double *rconst)
{
    extern __shared__ double e[];
    __shared__ double part[4];
    const int b = blockIdx.x, mdl = model_idx ? model_idx[b] : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const double *xb = x0 + (size_t)b * nx, *wb = omega + (size_t)b * nW;
    for (int i = wave; i < len; i += nwv) {
        double acc = 0.0;
        if (Mx) { const double *r = Mx + (size_t)mdl * sMx + (size_t)i * nx; for (int k = lane; k < nx; k += 64) acc += r[k] * xb[k]; }
        if (Mw) { const double *r = Mw + (size_t)mdl * sMw + (size_t)i * nW; for (int k = lane; k < nW; k += 64) acc += r[k] * wb[k]; }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if (lane == 0) e[i] = acc + (m0 ? m0[(size_t)mdl * sm0 + i] : 0.0);
    }
    __syncthreads();
    double tot = 0.0;
    const double *Wm = W + (size_t)mdl * len * len;
    for (int i = wave; i < len; i += nwv) {
        double acc = 0.0;
        for (int k = lane; k < len; k += 64) acc += Wm[(size_t)i * len + k] * e[k];
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if (lane == 0) tot += acc * e[i];
    }
    if (lane == 0) part[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) { double s = 0; for (int q = 0; q < nwv; ++q) s += part[q]; rconst[b] += s; }
}

// Ps = diag(cs) P diag(cs)
__global__ void k_scale_P(int n, const double *P, const double *cs, double *Ps)
{
    const int mdl = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (size_t)n * n) { const size_t i = e / n, j = e % n; Ps[(size_t)mdl * n * n + e] = P[(size_t)mdl * n * n + e] * cs[(size_t)mdl * n + i] * cs[(size_t)mdl * n + j]; }
}

// Receding horizon on device (one MPC step of the closed loop): the plant update the reference performs after every solve,
// ControllerBase.sim_step_k -> MldModel.lsim_k  x(k+1) = A x + B1 u + B2 delta + B3 z + B4 omega + b5  (controllers/
// controller_base.py:229-253, models/mld_model.py:647-699), with (u, delta, z) the step-0 slice of the solution just computed,
// and the disturbance forecast moved on by one step (the oldest step re-enters at the end of the horizon: the synthetic
// profiles are periodic).  One thread per (instance, state); writes the spare x0 / omega buffers (swapped by the host).
// an instance has a usable plan when its solve ended OPTIMAL, or at a limit with an incumbent (finite objective)
__device__ __forceinline__ bool plan_usable(const int *status, const double *obj, int b)
{
    const int s = status[b];
    return (s == MLD_STATUS_OPTIMAL || s == MLD_STATUS_NODE_LIMIT) && fabs(obj[b]) < 1.0e300;
}

__global__ void __launch_bounds__(256) k_advance(int batch, int nx, int nv, int nw, int N, const double *pack, size_t pack_len, int model_stride,
                                                size_t oA, size_t oB4, size_t ob5, size_t oBv, const int *model_idx, const double *x0,
                                                const double *omega, const double *v, size_t v_stride, double *x0_new, double *omega_new,
                                                const int *status, const double *obj, int *n_skipped)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nW = (size_t)N * nw;
    if (t < (size_t)batch && !plan_usable(status, obj, (int)t)) atomicAdd(n_skipped, 1);
    if (t < (size_t)batch * nx) {
        const int b = (int)(t / nx), i = (int)(t % nx);
        if (!plan_usable(status, obj, b)) { x0_new[t] = x0[t]; }      // no plan: the plant of this instance is not advanced
        else {
        const int mdl = (model_idx ? model_idx[b] : 0) * model_stride;
        const double *pk = pack + (size_t)mdl * pack_len;
        const double *xb = x0 + (size_t)b * nx, *wb = omega + (size_t)b * nW, *vb = v + (size_t)b * v_stride;
        double s = pk[ob5 + i];
        for (int j = 0; j < nx; ++j) s += pk[oA + (size_t)i * nx + j] * xb[j];
        for (int j = 0; j < nv; ++j) s += pk[oBv + (size_t)i * nv + j] * vb[j];
        for (int j = 0; j < nw; ++j) s += pk[oB4 + (size_t)i * nw + j] * wb[j];
        x0_new[t] = s;
        }
    }
    for (size_t e = t; e < (size_t)batch * nW; e += (size_t)gridDim.x * blockDim.x) {
        const size_t b = e / nW, r = e % nW;
        const size_t k = r / nw, c = r % nw;
        omega_new[e] = plan_usable(status, obj, (int)b) ? omega[b * nW + ((k + 1) % N) * nw + c] : omega[e];
    }
}

// MIP start from the last solution (mld_warm_start_from_previous): binary k of instance b takes the rounded value of the same per-step
// variable `shift` steps later in the previous plan (the last step repeats); instances without an incumbent get none (first byte 255)
__global__ void __launch_bounds__(256) k_warm_from_plan(int batch, int nb, int nv, int N, int shift, const int *bins, const double *v, size_t v_stride,
                                                       const int *status, const double *obj, unsigned char *warm)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)batch * nb) return;
    const int b = (int)(t / nb), k = (int)(t % nb);
    if (!plan_usable(status, obj, b)) { warm[t] = 255; return; }
    const int j = bins[k], step = j / nv, pos = j - step * nv;
    const int src = min(step + shift, N - 1);
    const double val = v[(size_t)b * v_stride + (size_t)src * nv + pos];
    warm[t] = val > 0.5 ? 1 : 0;
}

#include "trajectory.inc"      // k_trajectory / k_trajectory_valu (mld_predict_batch): they mask with plan_usable, like k_advance
#include "evaluate.inc"        // k_evaluate / k_evaluate_valu, k_eval_point, k_eval_obj (mld_evaluate_batch): the same masking
#include "sim_step.inc"        // k_sim_step (mld_sim_step_batch): lsim_k with the whole step-0 slice, the same masking

// ------------------------------------------------------------------------------------------------
/* buffers of the uploaded batch (ensure_batch, mld_upload_batch, mld_upload_constraint_blocks, mld_stage_inputs): released together when the
 * batch is laid out anew.  Inputs have one entry per instance, results one per queue entry (instances, then the items of the in-kernel hand-off). */
struct BatchBufs {
    DevBuf<int> model_idx; DevBuf<double> x0, omega, hs, qs_inst, rconst;
    DevBuf<double> x0b, omegab; DevBuf<int> skipped;     /* spare input buffers and device counter of mld_advance_batch (the counter: also the hand-off merge's) */
    DevBuf<unsigned char> warm; DevBuf<int> order;       /* MIP start (mld_set_warm_start); longest-first work-queue order learnt from the previous solve */
    DevBuf<unsigned char> fixed; DevBuf<double> cutoff, v, obj, lbnd;
    DevBuf<int> status, nodes, pivots, cuts, refac; DevBuf<long long> ticks, rows, prof;
    DevBuf<int> open_depth; DevBuf<short> open_var; DevBuf<unsigned char> open_val, open_flag;   /* open-node stacks (mld_download_open_nodes) */
    DevBuf<double> stage_x0, stage_om;                   /* resident input sets (mld_stage_inputs) */
    DevBuf<int> perm; DevBuf<RhsGroup> groups;           /* instances grouped by model for the MFMA right-hand sides (K3) */
    DevBuf<double> xcols, xcols_x; DevBuf<int> xrows;    /* extra constraint blocks; the state every extra column was generated with (explicit x_k) */
    DevBuf<double> sim_tmp;                              /* scratch of k_sim_step where its staging does not fit LDS: in_cap x (nomega + ny), on first use */
    DevBuf<double> icost, qs_inst_t;                     /* per-instance linear cost (mld_upload_instance_cost): batch x ic_ld, unscaled, pulled back to v
                                                            [then cx | cw | c0]; qs_inst under the Toeplitz-compatible column scales (k_lp_lds, on first use) */
    struct Handoff {      /* in-kernel sub-tree hand-off queue: allocated only while mld_set_handoff has it on */
        DevBuf<int> tail, finished, item_src, item_root, item_gen, item_ready, item_children; DevBuf<long long> item_label;
        DevBuf<unsigned long long> mg_best, mg_lbopen, mg_label; DevBuf<int> mg_open;   /* merge accumulators per root */
        DevBuf<int> tree_count, tree_dead;                /* items published per tree / tree given up */
    } ho;
};

/* what mld_solve_finish has to do: nothing launched; a dense solve queued on the stream; or an LDS-path solve that ran to completion in the
 * launch (the fall-back needs its statuses on the host), whose finish only reports */
enum class Flight : unsigned char { idle, queued, lds_done };

struct mld_problem {
    mld_model *model = nullptr;                 // caller's (original) model: used by mld_rhs_batch
    std::unique_ptr<mld_model> tight;           // internal copy with tightened rows, condensed on device
    mld_opts opts{};
    int N_p = 0, N = 0, n = 0, m0 = 0, nb = 0, nx = 0, nW = 0, nv = 0, n_models = 0;
    void *h_trace = nullptr; int *d_trace = nullptr; size_t trace_bytes = 0;   /* mld_debug_trace: file-backed host buffer the kernel writes its stage markers into */
    int mir_cap = 0;            /* integer entries of the widest scaled original row over all models, rounded up to 8 (k_solve's compact c-MIR lines) */
    SolverShape S{};
    unsigned slot_mask = 0;     /* MLD_SOL_SLOT at creation: the hot arrays build_shape kept in the slot (bit k: SLOT_NAMES[k]) */
    // per-model device arrays
    DevBuf<double> d_Gp;        /* d_Gs with columns in dictionary (position-major) order: coalesced dictionary reset */
    DevBuf<double> d_actmax;    /* n_models x m0: largest row activity under the model's bounds (s_mark_dead) */
    /* sparse copies of the scaled rows for the per-instance presolve (s_presolve): by row and by column, nnz_cap entries per model */
    DevBuf<int> d_csr_ptr, d_csc_ptr; DevBuf<unsigned short> d_csr_col, d_csc_row; DevBuf<double> d_csr_val, d_csc_val; int nnz_cap = 0;
    DevBuf<double> d_Gs, d_rs, d_cs, d_qs, d_lb, d_ub, d_cx, d_cw, d_c0, d_q0;
    DevBuf<unsigned char> d_is_int;
    DevBuf<int> d_bins, d_colperm, d_binpos;   /* d_binpos: position of a structural among the binaries, -1 for continuous entries (in-kernel hand-off) */
    // quadratic cost (K4)
    DevBuf<double> d_P, d_Qx, d_Qw, d_Ps, d_Wx, d_Wy;
    bool has_quad = false;
    // workspace
    DevBuf<unsigned char> d_ws; DevBuf<int> d_counter;
    int n_slots = 0;
    size_t lds_bytes = 0;
    // batch buffers, and what they hold: every per-entry result array has batch_cap entries, the inputs in_cap
    BatchBufs bat;
    int batch = 0, batch_cap = 0, in_cap = 0;
    bool has_fixed = false, has_midx = false, has_warm = false;
    bool solved = false;        /* the resident batch has a finished solve (mld_advance_batch / mld_warm_start_from_previous need one) */
    bool advanced = false;      /* mld_advance_batch has applied that solve's plan: the next advance needs the next solve */
    bool has_cutoff = false, want_open = false;    /* objective cutoffs (mld_set_cutoffs); record the open-node stacks (mld_record_open_nodes) */
    int n_staged = 0, staged_batch = 0, n_groups = 0, n_xcols = 0, order_batch = 0; size_t xcols_cap = 0; bool has_xcols_x = false;
    int ic_ld = 0;              /* row length of bat.icost: 0 = no per-instance cost resident, n = weights on v only, n + nx + nW + 1 = with the constant's maps */
    DevBuf<double> d_gather; size_t gather_cap = 0;   /* send + receive buffers of mld_gather_results */
    /* LDS-resident LP path (k_lp_lds): Toeplitz-compatible scaling of the tightened model */
    bool lp_ok = false, all_fixed = false; LpShape LS{}; size_t lp_lds_bytes = 0; int lp_slots = 0;
    DevBuf<double> d_blk_t, d_rs_t, d_cs_t, d_lb_t, d_ub_t, d_qs_t;
    hipEvent_t ev[3] = {}; bool ev_ok = false; DevBuf<long long> d_statbuf;
    hipStream_t stream = 0; bool own_stream = false; Flight flight = Flight::idle;   /* stream of the solve path (0 = the legacy stream); a launched, not yet finished solve */
    bool std_block = true;      /* the standard constraint block (right-hand side from the batch's own omega) is part of the problem (mld_set_std_block) */
    /* in-kernel sub-tree hand-off (mld_set_handoff) */
    int ho_enable = 0, ho_sub_nodes = 0, ho_max_gen = 0, ho_max_children = 0; double ho_factor = 2.0; bool ho_ran = false;
    int ho_max_tree = 160, ho_donate = 0, ho_rounds = 0;   /* items per tree; shallow open nodes handed off per node-limit, times */
    /* resident disturbance profiles (mld_upload_profiles): owned by the problem, not by the batch -- free_batch leaves them alone.  The start arrays belong
     * to a batch SIZE (pf_fbatch / pf_cbatch, 0 = none resident); per group the largest resident start is kept on the host, so that a call with
     * start == NULL is checked against the window rule without reading the device */
    DevBuf<double> pf_lib; long long pf_len = 0; int pf_groups = 0; std::vector<int> pf_width; DevBuf<PfChan> pf_chan;
    DevBuf<long long> pf_fstart, pf_cstart; int pf_fbatch = 0, pf_cbatch = 0, pf_ccols = 0; std::vector<long long> pf_fmax, pf_cmax;
    DevBuf<long long> pf_astart; int pf_abatch = 0; std::vector<long long> pf_amax;      /* starts of the REALISED series (mld_sim_step_batch, MLD_SIM_ACTUAL): an array of their own */
    /* resident simulation log (mld_sim_log_begin): `cap` records of the resident batch, one array per field, each (cap, batch, width).  It belongs to the
     * resident batch: mld_upload_batch discards it */
    struct SimLog {
        DevBuf<double> x, v, y, om, x_k1, vio, obj, lb; DevBuf<unsigned char> cons; DevBuf<int> row, status, nodes;
        int cap = 0, count = 0;
    } slog;
    long long ho_stats[4] = {};  /* last solve: items published, trees split, trees left unfinished, entries the queue had no room for (always 0: such trees stay unfinished) */
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* mld_opts.time_limit (seconds) in ticks of the device's constant wall clock (wall_clock64: 100 MHz on gfx950) */
static long long time_limit_ticks(double seconds)
{
    if (!(seconds > 0.0)) return 0;
    int dev = 0, khz = 100000;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
    const double t = seconds * 1.0e3 * (double)khz;
    return t >= 9.0e18 ? (long long)9.0e18 : (long long)std::max(1.0, t);
}

/* MLD_SOL_SLOT (diagnostics and tests): a comma list of the hot arrays that stay in the slot even where they would fit in LDS, or "all"; the rest of the
 * placement ladder runs as before.  Read when the problem is created (build_shape); an unknown name is an error, so that a typo cannot test the default. */
static const char *const SLOT_NAMES[] = {"xb", "basic", "skip", "atup", "nonbasic", "xn", "lohi", "dw", "cost", "mirline", "mircache"};
enum { SLOT_N = (int)(sizeof(SLOT_NAMES) / sizeof(SLOT_NAMES[0])) };

static int sol_slot_mask(unsigned *mask)
{
    *mask = 0;
    const char *env = getenv("MLD_SOL_SLOT");
    if (!env) return MLD_OK;
    const std::string all(env);
    size_t b = 0;
    while (b <= all.size()) {
        size_t e = all.find(',', b);
        if (e == std::string::npos) e = all.size();
        const std::string name = all.substr(b, e - b);
        int k = 0;
        if (name == "all") *mask |= (1u << SLOT_N) - 1u;
        else if (!name.empty()) {
            while (k < SLOT_N && name != SLOT_NAMES[k]) ++k;
            if (k == SLOT_N) { mld_set_error("MLD_SOL_SLOT: unknown array '%s' (xb, basic, skip, atup, nonbasic, xn, lohi, dw, cost, mirline, mircache, all)", name.c_str()); return MLD_ERR_INVALID; }
            *mask |= 1u << k;
        }
        b = e + 1;
    }
    return MLD_OK;
}

static int build_shape(mld_problem *p)
{
    unsigned slot = 0;
    if (int rc = sol_slot_mask(&slot)) return rc;
    p->slot_mask = slot;
    SolverShape &S = p->S;
    const mld_opts &o = p->opts;
    /* cut rows: max_cuts for the root cut loop + S_RESTART_ROWS (0) that only the root restart may use (k_solve: more cut rounds at the root once an incumbent leaves a
     * small gap; the first loop needs its max_cuts -- capping it lower to make room measured +37 % row updates on the steady-state instances) */
    const int restart_rows = (o.max_cuts > 0 && o.cut_rounds > 0) ? S_RESTART_ROWS : 0;
    S.n = p->n; S.m0 = p->m0; S.mcap = p->m0 + o.max_cuts + restart_rows; S.first_cap = p->m0 + o.max_cuts; S.ld = (p->n + 1 + 7) & ~7;   /* rows start on 64-byte sectors */
    S.ntot = p->n + S.mcap;
    S.nb = p->nb; S.nx = p->nx; S.nW = p->nW; S.N = p->N; S.nv = p->nv;
    S.max_cuts = o.max_cuts; S.cuts_per_round = o.cuts_per_round; S.cut_rounds = o.cut_rounds;
    S.max_nodes = o.max_nodes; S.max_pivots = o.max_pivots; S.gap_abs = o.gap_abs; S.gap_rel = o.gap_rel;
    S.debug = o.reserved;
    S.presolve = (o.presolve & 4) && p->m0 < 65536 && p->n < 65536 ? 1 : 0;
    S.time_ticks = time_limit_ticks(o.time_limit);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t r = off; off = align_up(off + bytes, 256); return r; };
    const size_t n = S.n, mc = S.mcap, nt = S.ntot, nb = std::max(1, S.nb);
    S.oD = take(sizeof(double) * (mc + 1) * S.ld);
    S.oGc = take(sizeof(double) * std::max<size_t>(1, o.max_cuts + restart_rows) * n);
    S.oHc = take(sizeof(double) * std::max<size_t>(1, o.max_cuts + restart_rows));
    S.oLo = take(sizeof(double) * nt); S.oHi = take(sizeof(double) * nt);
    S.oXB = take(sizeof(double) * mc); S.oXN = take(sizeof(double) * n);
    S.oBasic = take(sizeof(int) * mc); S.oNonbasic = take(sizeof(int) * n); S.oWhere = take(sizeof(int) * nt);
    S.oAtUp = take(n); S.oSkip = take(mc);
    S.oTmpX = take(sizeof(double) * n); S.oG = take(sizeof(double) * n); S.oAx = take(sizeof(double) * n);
    S.oRootLo = take(sizeof(double) * n); S.oRootHi = take(sizeof(double) * n);
    S.oStkJ = take(sizeof(int) * (nb + 2)); S.oStkF = take(nb + 2); S.oStkS = take(nb + 2);
    S.oSvJ = take(sizeof(int) * (nb + 2)); S.oSvLo = take(sizeof(double) * (nb + 2)); S.oSvHi = take(sizeof(double) * (nb + 2));
    S.oKey = take(sizeof(double) * std::max<size_t>(std::max<size_t>(mc, nb + 2), 64)); S.oXo = take(sizeof(double) * n);
    S.oY = take(sizeof(double) * 33 * n); S.oPY = take(sizeof(double) * 33 * n);
    S.oHm = take(sizeof(double) * 32 * 32); S.oCm = take(sizeof(double) * 32); S.oWm = take(sizeof(double) * 32);
    S.oGcost = take(sizeof(double) * n); S.oVcur = take(sizeof(double) * n); S.oPv = take(sizeof(double) * n);
    S.oXroot = take(sizeof(double) * (nb + 2)); S.oFxLo = take(sizeof(double) * (nb + 2)); S.oFxHi = take(sizeof(double) * (nb + 2));
    S.oFxJ = take(sizeof(int) * (nb + 2));
    S.oMirEff = take(sizeof(double) * std::max<size_t>(1, S.m0)); S.oMirDelta = take(sizeof(double) * std::max<size_t>(1, S.m0));
    S.oMirCache = take(sizeof(double) * SOL_NW * 2 * n);
    S.oDw = take(sizeof(double) * mc);
    S.oLive = take(sizeof(unsigned short) * std::max<size_t>(8, S.m0));
    S.oMq = take(sizeof(double) * SD_MQ_DOUBLES);      /* work arrays of the master QP (simplicial decomposition) */
    S.oClo = take(sizeof(double) * n); S.oChi = take(sizeof(double) * n);      /* bounds the cut builders may use for the continuous structurals (s_presolve) */
    S.oStkV = take(nb + 2);                             /* the search path's values while a stopped search closes its open siblings (in-kernel hand-off) */
    S.mir_per_round = o.mir_per_round;
    S.ws_stride = align_up(off, 4096);
    S.seccap = (int)std::max<size_t>(std::max<size_t>(mc + 8, n + 8), (n + SOL_SEC) / SOL_SEC + 8);      /* (also the list of the columns the long-step ratio test flips: up to n) */
    p->lds_bytes = sizeof(double) * (n + 2 + mc + 2 + n + 2) + sizeof(unsigned short) * ((size_t)S.seccap + mc + 8 + 8);
    /* hot per-basis state moves from the slot into LDS while it fits (one workgroup per CU: 160 KB LDS) */
    size_t loff = align_up(p->lds_bytes, 16);
#ifndef SOL_LDS_BUDGET
#define SOL_LDS_BUDGET ((SOL_WPE >= 4 ? 78 : 144) * 1024)
#endif
    const size_t budget = SOL_LDS_BUDGET;
    /* k: the array's bit in the MLD_SOL_SLOT mask (SLOT_NAMES) */
    auto ltake = [&](size_t bytes, int k) -> int { const size_t b = align_up(bytes, 16); if ((slot >> k & 1u) || loff + b > budget) return -1; const size_t r = loff; loff += b; return (int)r; };
    S.lXB = ltake(sizeof(double) * mc, 0); S.lBasic = ltake(sizeof(int) * mc, 1); S.lSkip = ltake(mc, 2);
    S.lAtUp = ltake(n, 3); S.lNonbasic = ltake(sizeof(int) * n, 4); S.lXN = ltake(sizeof(double) * n, 5);
    S.lLo = ltake(sizeof(double) * nt, 6); S.lHi = S.lLo >= 0 ? ltake(sizeof(double) * nt, 6) : -1;
    S.lDw = ltake(sizeof(double) * mc, 7);
    S.lCost = ltake(sizeof(double) * (n + 1), 8);                     /* the reduced-cost row: read by every ratio test, updated by every pivot */
    S.mir_cap = p->mir_cap; S.lMirLine = -1;
    if (p->mir_cap > 0 && p->mir_cap < n) S.lMirLine = ltake(sizeof(double) * SOL_NW * 2 * p->mir_cap, 9);  /* compact lines of the c-MIR scoring (a row's free binaries) */
    S.lMirCache = ltake(sizeof(double) * SOL_NW * 2 * n, 10);                                              /* full-width lines (Gomory rounds): LDS while it fits */
    /* Buffers of the second pivot of a fused pair (s_pivot_pair): row, multiplier column, union lists, sector flags.  They need no bytes of their own: the per-wave
     * lines of lMirCache are scratch of the cut rounds and dead while the dual simplex runs, so the pair's buffers lie over them when every hot array is in LDS. */
    {
        const bool all_lds = S.lXB >= 0 && S.lXN >= 0 && S.lLo >= 0 && S.lHi >= 0 && S.lBasic >= 0 && S.lNonbasic >= 0 && S.lAtUp >= 0 && S.lSkip >= 0 && S.lDw >= 0 && S.lCost >= 0;
        S.lPair = (all_lds && S.lMirCache >= 0 && pair_lds_bytes(S.n, S.mcap) <= sizeof(double) * SOL_NW * 2 * n) ? S.lMirCache : -1;
    }
    p->lds_bytes = loff;
    return MLD_OK;
}

/* a host array to a buffer of its own size (an empty array leaves the buffer empty) */
template <typename T> static int upload(DevBuf<T> &dst, const std::vector<T> &src)
{
    if (src.empty()) { dst.reset(); return MLD_OK; }
    HIP_TRY(dst.alloc(src.size()));
    HIP_TRY(hipMemcpy(dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    return MLD_OK;
}

/* a launched solve (mld_solve_launch) owns the problem's buffers until mld_solve_finish */
#define MLD_NOT_IN_FLIGHT(p, who) do { if ((p) && (p)->flight != Flight::idle) { mld_set_error("%s: a launched solve has not been finished (mld_solve_finish)", who); return MLD_ERR_INVALID; } } while (0)

static void free_batch(mld_problem *p)
{
    p->bat = BatchBufs();
    if (p->slog.cap) p->slog = mld_problem::SimLog();
    p->n_groups = 0; p->has_warm = false; p->solved = false; p->advanced = false; p->has_cutoff = false;
    p->n_staged = 0; p->staged_batch = 0; p->n_xcols = 0; p->xcols_cap = 0; p->has_xcols_x = false;
    p->order_batch = 0; p->in_cap = 0; p->batch_cap = 0; p->ic_ld = 0;
}

// out[k] = a[k] * b[k]
__global__ void __launch_bounds__(256) k_scale_vec(size_t count, const double *a, const double *b, double *out)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) out[k] = a[k] * b[k];
}

static int set_cost_impl(mld_problem *p, const mld_cost *cost)
{
    const int n = p->n, M = p->n_models, nx = p->nx, nW = p->nW;
    const int NX = p->N * p->model->dims.nx, NY = p->N * p->model->dims.ny;
    const mld_model *t = p->tight.get();
    /* Everything runs on the problem's own stream and ends with a wait on THAT stream: a caller that updates the cost of one problem every step
     * (the reference rebuilds its objective with the new prices before every solve, micro_grid_control_simulation.py:197-198,229) must not stall
     * the solve another problem has in flight.  A purely linear cost on v (lin_v only: the bench's q_z / q_mu atoms) needs no temporary and no
     * host round trip: upload, scale on the device. */
    const hipStream_t sq = p->stream;
    // q0 = lin_v + Gamma_v' lin_x + L_v' lin_y ; cx = Phi' lin_x + L_x' lin_y ; cw = Gamma_w' lin_x + L_w' lin_y ; c0 = ...
    HIP_TRY(hipMemsetAsync(p->d_q0, 0, sizeof(double) * n * M, sq));
    HIP_TRY(hipMemsetAsync(p->d_cx, 0, sizeof(double) * std::max(1, nx) * M, sq));
    HIP_TRY(hipMemsetAsync(p->d_cw, 0, sizeof(double) * std::max(1, nW) * M, sq));
    HIP_TRY(hipMemsetAsync(p->d_c0, 0, sizeof(double) * M, sq));
    if (cost && cost->lin_v) HIP_TRY(hipMemcpyAsync(p->d_q0, cost->lin_v, sizeof(double) * n * M, hipMemcpyHostToDevice, sq));
    auto pull = [&](const double *hw, int len, int oV, int oX, int oW, int o5) -> int {
        if (!hw || len == 0) return MLD_OK;
        DevBuf<double> d_w;      /* (released on every return path) */
        HIP_TRY(d_w.alloc((size_t)len * M));
        HIP_TRY(hipMemcpyAsync(d_w, hw, sizeof(double) * len * M, hipMemcpyHostToDevice, sq));
        const dim3 blk(256);
        if (t->d_out[oV]) hipLaunchKernelGGL(k_pullback, dim3((n + 255) / 256, M), blk, 0, sq, len, n, t->d_out[oV], t->lay.out_size[oV], d_w, (size_t)len, p->d_q0, (size_t)n, 1);
        if (nx && t->d_out[oX]) hipLaunchKernelGGL(k_pullback, dim3((nx + 255) / 256, M), blk, 0, sq, len, nx, t->d_out[oX], t->lay.out_size[oX], d_w, (size_t)len, p->d_cx, (size_t)nx, 1);
        if (nW && t->d_out[oW]) hipLaunchKernelGGL(k_pullback, dim3((nW + 255) / 256, M), blk, 0, sq, len, nW, t->d_out[oW], t->lay.out_size[oW], d_w, (size_t)len, p->d_cw, (size_t)nW, 1);
        if (t->d_out[o5]) hipLaunchKernelGGL(k_pullback, dim3(1, M), blk, 0, sq, len, 1, t->d_out[o5], t->lay.out_size[o5], d_w, (size_t)len, p->d_c0, (size_t)1, 1);
        HIP_TRY(hipStreamSynchronize(sq));      /* (the temporary is released when this scope ends) */
        return MLD_OK;
    };
    int rc;
    if (cost) {
        if ((rc = pull(cost->lin_x, NX, O_GamV, O_PhiX, O_GamW, O_Gam5))) return rc;
        if ((rc = pull(cost->lin_y, NY, O_LV, O_LX, O_LW, O_L5))) return rc;
    }
    // quadratic part (assembled for mld_cost_assemble; the MILP solver rejects it)
    p->has_quad = cost && (cost->quad_v || cost->quad_x || cost->quad_y);
    p->d_P.reset(); p->d_Qx.reset(); p->d_Qw.reset(); p->d_Ps.reset(); p->d_Wx.reset(); p->d_Wy.reset();
    if (p->has_quad) {
        HIP_TRY(p->d_P.alloc((size_t)n * n * M));
        HIP_TRY(hipMemset(p->d_P, 0, sizeof(double) * (size_t)n * n * M));
        if (nx) { HIP_TRY(p->d_Qx.alloc((size_t)n * nx * M)); HIP_TRY(hipMemset(p->d_Qx, 0, sizeof(double) * (size_t)n * nx * M)); }
        if (nW) { HIP_TRY(p->d_Qw.alloc((size_t)n * nW * M)); HIP_TRY(hipMemset(p->d_Qw, 0, sizeof(double) * (size_t)n * nW * M)); }
        if (cost->quad_v) {
            DevBuf<double> d_W, d_Ws;
            HIP_TRY(d_W.alloc((size_t)n * n * M)); HIP_TRY(d_Ws.alloc((size_t)n * n * M));
            HIP_TRY(hipMemcpyAsync(d_W, cost->quad_v, sizeof(double) * (size_t)n * n * M, hipMemcpyHostToDevice, sq));
            hipLaunchKernelGGL(k_symmetrize, dim3(((size_t)n * n + 255) / 256, M), dim3(256), 0, sq, n, d_W, d_Ws, (size_t)n * n);
            HIP_TRY(hipMemcpyAsync(p->d_P, d_Ws, sizeof(double) * (size_t)n * n * M, hipMemcpyDeviceToDevice, sq));
            HIP_TRY(hipStreamSynchronize(sq));
        }
        auto quad = [&](const double *hW, int len, int oV, int oX, int oW, int o5, DevBuf<double> &keepW) -> int {
            if (!hW || len == 0) return MLD_OK;
            const size_t ll = (size_t)len * len;
            DevBuf<double> d_W, d_Ws, d_T;
            HIP_TRY(d_W.alloc(ll * M)); HIP_TRY(d_Ws.alloc(ll * M));
            const size_t tcols = (size_t)std::max(std::max(n, nx), std::max(nW, 1));     /* d_T also holds the len x nx and len x nW products */
            HIP_TRY(d_T.alloc((size_t)len * tcols * M));
            HIP_TRY(hipMemcpyAsync(d_W, hW, sizeof(double) * ll * M, hipMemcpyHostToDevice, sq));
            hipLaunchKernelGGL(k_symmetrize, dim3((ll + 255) / 256, M), dim3(256), 0, sq, len, d_W, d_Ws, ll);
            // T = Ws * Mv (len x n) ; P += Mv' T ; Qx += (Ws Mx)' ... computed as Mv' (Ws Mx)
            const dim3 blk(256);
            auto gemm = [&](int Mm, int Nn, int K, int tA, const double *A, size_t sA, const double *Bp, size_t sB, double *Cp, size_t sC, double beta) {
                if (p->opts.reserved & MLD_DBG_GEMM_VALU) hipLaunchKernelGGL(k_gemm, dim3((Nn + 15) / 16, (Mm + 15) / 16, M), blk, 0, sq, Mm, Nn, K, tA, A, sA, Bp, sB, Cp, sC, 1.0, beta);
                else if (p->opts.flags & MLD_F32) hipLaunchKernelGGL(k_gemm_mfma<true>, dim3((Nn + GM_T - 1) / GM_T, (Mm + GM_T - 1) / GM_T, M), blk, 0, sq, Mm, Nn, K, tA, A, sA, Bp, sB, Cp, sC, 1.0, beta);
                else hipLaunchKernelGGL(k_gemm_mfma<false>, dim3((Nn + GM_T - 1) / GM_T, (Mm + GM_T - 1) / GM_T, M), blk, 0, sq, Mm, Nn, K, tA, A, sA, Bp, sB, Cp, sC, 1.0, beta);
            };
            if (t->d_out[oV]) {
                gemm(len, n, len, 0, d_Ws, ll, t->d_out[oV], t->lay.out_size[oV], d_T, (size_t)len * tcols, 0.0);
                gemm(n, n, len, 1, t->d_out[oV], t->lay.out_size[oV], d_T, (size_t)len * tcols, p->d_P, (size_t)n * n, 1.0);
                if (nx && t->d_out[oX]) {
                    gemm(len, nx, len, 0, d_Ws, ll, t->d_out[oX], t->lay.out_size[oX], d_T, (size_t)len * tcols, 0.0);
                    gemm(n, nx, len, 1, t->d_out[oV], t->lay.out_size[oV], d_T, (size_t)len * tcols, p->d_Qx, (size_t)n * nx, 1.0);
                }
                if (nW && t->d_out[oW]) {
                    gemm(len, nW, len, 0, d_Ws, ll, t->d_out[oW], t->lay.out_size[oW], d_T, (size_t)len * tcols, 0.0);
                    gemm(n, nW, len, 1, t->d_out[oV], t->lay.out_size[oV], d_T, (size_t)len * tcols, p->d_Qw, (size_t)n * nW, 1.0);
                }
                if (t->d_out[o5]) {
                    gemm(len, 1, len, 0, d_Ws, ll, t->d_out[o5], t->lay.out_size[o5], d_T, (size_t)len * tcols, 0.0);
                    gemm(n, 1, len, 1, t->d_out[oV], t->lay.out_size[oV], d_T, (size_t)len * tcols, p->d_q0, (size_t)n, 1.0);
                }
            }
            HIP_TRY(hipStreamSynchronize(sq));
            keepW = std::move(d_W);      // un-symmetrised weight, kept for the objective constant e'We
            return MLD_OK;
        };
        if ((rc = quad(cost->quad_x, NX, O_GamV, O_PhiX, O_GamW, O_Gam5, p->d_Wx))) return rc;
        if ((rc = quad(cost->quad_y, NY, O_LV, O_LX, O_LW, O_L5, p->d_Wy))) return rc;
        HIP_TRY(p->d_Ps.alloc((size_t)n * n * M));
        hipLaunchKernelGGL(k_scale_P, dim3(((size_t)n * n + 255) / 256, M), dim3(256), 0, sq, n, p->d_P, p->d_cs, p->d_Ps);
    }
    // scaled cost for the solver: qs = q0 .* cs (and with the Toeplitz-compatible column scales for the LDS-resident LP path)
    const size_t tot = (size_t)n * M;
    if (tot) {
        hipLaunchKernelGGL(k_scale_vec, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, sq, tot, p->d_q0, p->d_cs, p->d_qs);
        if (p->lp_ok) hipLaunchKernelGGL(k_scale_vec, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, sq, tot, p->d_q0, p->d_cs_t, p->d_qs_t);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sq));
    return MLD_OK;
}

extern "C" {

/* sizeof(mld_opts) of THIS build: a binding compiled against another layout of the struct must not call mld_problem_create (checked by the Python loader) */
int mld_opts_size(void) { return (int)sizeof(mld_opts); }

int mld_opts_default(mld_opts *o)
{
    if (!o) return MLD_ERR_INVALID;
    o->gap_abs = 1e-9; o->gap_rel = 0.0; o->max_nodes = 100000; o->max_pivots = 50000; o->cut_rounds = -1;
    o->cuts_per_round = -1; o->max_cuts = -1; o->presolve = 6; o->n_slots = 0; o->mir_per_round = -1; o->flags = 0; o->reserved = 0; o->time_limit = 0.0;
    return MLD_OK;
}

/* the device buffers release themselves with the handle; the solve path's stream is drained first (a queued kernel may still use them and the trace) */
int mld_problem_destroy(mld_problem_t *p)
{
    if (!p) return MLD_OK;
    (void)hipStreamSynchronize(p->stream);
    if (p->ev_ok) { (void)hipEventDestroy(p->ev[0]); (void)hipEventDestroy(p->ev[1]); (void)hipEventDestroy(p->ev[2]); }
    if (p->own_stream) (void)hipStreamDestroy(p->stream);
    if (p->h_trace) { (void)hipHostUnregister(p->h_trace); munmap(p->h_trace, p->trace_bytes); }
    delete p;
    return MLD_OK;
}

int mld_problem_create(mld_problem_t **out, mld_model_t *model, int N_p, int N_tilde, const mld_cost *cost,
                       const mld_opts *opts)
{
    if (!out || !model || N_tilde < 1) { mld_set_error("mld_problem_create: bad arguments"); return MLD_ERR_INVALID; }
    std::unique_ptr<mld_problem, int (*)(mld_problem_t *)> p(new mld_problem(), mld_problem_destroy);      /* (every error return releases it) */
    p->model = model;
    if (opts) p->opts = *opts; else mld_opts_default(&p->opts);
    const mld_dims &d = model->dims;
    p->N_p = N_p; p->N = N_tilde; p->nv = model->nv; p->n = N_tilde * model->nv; p->m0 = N_tilde * d.nc;
    {   /* cut budgets: a negative value asks for the size-scaled default (300 rows / 80 Gomory + 10 rounding cuts per round up to the cfg3
         * shape).  Round 1 ran 200 / 40 / 20 over 8 rounds and withdrew anything deeper after one false optimality claim; that claim was
         * the dual simplex's tiny-pivot breakdown (DESIGN section 4), and with the guard the deeper loop is clean against HiGHS
         * (tests/test_gpu_loop.py) and 5 % faster: Gomory cuts are derived eight at a time and nearly free, rounding cuts are not. */
        const int nbin = N_tilde * (d.nu_l + d.ndelta + d.nmu_l);
        /* round 3: 20 rounding cuts per round (was 10: 2048 bench instances on the CPU restatement: 12 % fewer row updates, 9 -> 3 node-limited;
         * steady-state closed-loop instances: 18 % fewer), and above the cfg4 size the loop deepens with the number of binaries -- cfg5 (784
         * binaries, NodeLimit 400, 256 instances): 10 rounds / 441 rows / 78 rounding cuts 47 % proven, 19 rounds / 882 rows / 156 rounding cuts 59 % */
        if (p->opts.max_cuts < 0) p->opts.max_cuts = nbin <= 400 ? std::max(300, p->m0 / 4) : p->m0 / 2;
        if (p->opts.cuts_per_round < 0) p->opts.cuts_per_round = std::max(80, nbin / 5);
        if (p->opts.mir_per_round < 0) p->opts.mir_per_round = nbin <= 400 ? 20 : nbin / 5;
        if (p->opts.cut_rounds < 0) p->opts.cut_rounds = std::max(10, std::min(30, nbin / 40));
    }
    if (p->opts.cut_rounds <= 0 || p->opts.max_cuts == 0) { p->opts.cut_rounds = 0; }
    p->nx = d.nx; p->nW = N_tilde * d.nomega; p->n_models = model->n_models;
    const int n = p->n, m0 = p->m0, M = p->n_models;
    int rc = MLD_OK;
    // 1. tightened copy of the model, condensed on device (K1+K2)
    {
        std::vector<std::vector<double>> hm = model->h_mats;
        const int steps = model->tv_N > 0 ? model->tv_N : 1;      /* time-varying horizon: every step model is tightened on its own rows */
        if (p->opts.presolve & 2) for (int k = 0; k < M * steps; ++k) tighten::run(d, hm, (size_t)k);
        const double *ptrs[20];
        for (int k = 0; k < 20; ++k) ptrs[k] = hm[k].empty() ? nullptr : hm[k].data();
        mld_model *t = nullptr;
        if ((rc = model_create_impl(&t, &d, M, model->tv_N, ptrs))) return rc;
        p->tight.reset(t);
        if ((rc = condense_model_device(t, N_tilde, nullptr, 0))) return rc;
    }
    // 2. variable layout: bounds + binaries  (variables.py:189-243 ; mld_model.py:294-345)
    std::vector<double> lb((size_t)n, -std::numeric_limits<double>::infinity()), ub((size_t)n, std::numeric_limits<double>::infinity());
    std::vector<unsigned char> is_int(n, 0);
    std::vector<int> bins;
    for (int k = 0; k < N_tilde; ++k) {
        const int o = k * p->nv;
        for (int j = d.nu - d.nu_l; j < d.nu; ++j) is_int[o + j] = 1;
        for (int j = 0; j < d.ndelta; ++j) is_int[o + d.nu + j] = 1;
        const int omu = d.nu + d.ndelta + d.nz;
        for (int j = 0; j < d.nmu; ++j) lb[o + omu + j] = 0.0;
        for (int j = d.nmu - d.nmu_l; j < d.nmu; ++j) is_int[o + omu + j] = 1;
    }
    for (int j = 0; j < n; ++j) if (is_int[j]) { lb[j] = 0.0; ub[j] = 1.0; bins.push_back(j); }
    p->nb = (int)bins.size();
    // 3. scaling from the tightened H_v (host, once per problem) and the scaled dense G
    std::vector<double> G((size_t)m0 * n * M), rs((size_t)m0 * M, 1.0), cs((size_t)n * M, 1.0);
    if (m0 && n) {
        hipError_t e = hipMemcpy(G.data(), p->tight->d_out[O_HV], sizeof(double) * G.size(), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { mld_set_error("D2H H_v: %s", hipGetErrorString(e)); return MLD_ERR_HIP; }
    }
    for (int k = 0; k < M; ++k) {
        double *g = G.data() + (size_t)k * m0 * n, *r = rs.data() + (size_t)k * m0, *c = cs.data() + (size_t)k * n;
        std::vector<double> cmax(n);
        for (int pass = 0; pass < 3; ++pass) {
            for (int i = 0; i < m0; ++i) {
                double mx = 0;
                for (int j = 0; j < n; ++j) mx = std::max(mx, std::fabs(g[(size_t)i * n + j]) * r[i] * c[j]);
                if (mx > 0) r[i] /= mx;
            }
            std::fill(cmax.begin(), cmax.end(), 0.0);
            for (int i = 0; i < m0; ++i)
                for (int j = 0; j < n; ++j) cmax[j] = std::max(cmax[j], std::fabs(g[(size_t)i * n + j]) * r[i] * c[j]);
            for (int j = 0; j < n; ++j) if (!is_int[j] && cmax[j] > 0) c[j] /= cmax[j];
        }
        for (int i = 0; i < m0; ++i) r[i] = std::exp2(std::rint(std::log2(r[i])));
        for (int j = 0; j < n; ++j) c[j] = std::exp2(std::rint(std::log2(c[j])));
        for (int i = 0; i < m0; ++i)
            for (int j = 0; j < n; ++j) g[(size_t)i * n + j] *= r[i] * c[j];
    }
    std::vector<double> lbs((size_t)n * M), ubs((size_t)n * M);
    for (int k = 0; k < M; ++k)
        for (int j = 0; j < n; ++j) { lbs[(size_t)k * n + j] = lb[j] / cs[(size_t)k * n + j]; ubs[(size_t)k * n + j] = ub[j] / cs[(size_t)k * n + j]; }
    if ((rc = upload(p->d_Gs, G)) || (rc = upload(p->d_rs, rs)) || (rc = upload(p->d_cs, cs)) || (rc = upload(p->d_lb, lbs)) ||
        (rc = upload(p->d_ub, ubs))) return rc;
    {
        int cap = 0;
        for (size_t r = 0; r < (size_t)M * m0; ++r) {
            int cnt = 0;
            for (int j = 0; j < n; ++j) cnt += (is_int[j] && G[r * n + j] != 0.0);
            cap = std::max(cap, cnt);
        }
        p->mir_cap = (cap + 7) / 8 * 8;
    }
    if (m0 && n) {   /* largest activity of every scaled row under the model's own bounds (k_solve's s_mark_dead compares it with the instance's right-hand side) */
        std::vector<double> am((size_t)m0 * M);
        for (int k = 0; k < M; ++k)
            for (int i = 0; i < m0; ++i) {
                const double *g = G.data() + ((size_t)k * m0 + i) * n;
                double act = 0.0; bool inf = false;
                for (int j = 0; j < n; ++j) {
                    const double gj = g[j];
                    if (gj > 0.0) { const double hi = ubs[(size_t)k * n + j]; if (hi < 0.5 * S_BIG) act += gj * hi; else inf = true; }
                    else if (gj < 0.0) { const double lo = lbs[(size_t)k * n + j]; if (lo > -0.5 * S_BIG) act += gj * lo; else inf = true; }
                }
                am[(size_t)k * m0 + i] = inf ? (double)INFINITY : act;
            }
        if ((rc = upload(p->d_actmax, am))) return rc;
    }
    if (m0 && n && (p->opts.presolve & 4) && m0 < 65536 && n < 65536) {
        /* the scaled rows once more, sparse (by row and by column): the per-instance presolve walks the non-zeros only (cfg4: 5 450 of 287 500) */
        size_t cap = 1;
        for (int k = 0; k < M; ++k) { size_t c = 0; const double *g = G.data() + (size_t)k * m0 * n; for (size_t e = 0; e < (size_t)m0 * n; ++e) c += g[e] != 0.0; cap = std::max(cap, c); }
        cap = (cap + 7) / 8 * 8;
        std::vector<int> rptr((size_t)M * (m0 + 1)), cptr((size_t)M * (n + 1));
        std::vector<unsigned short> rcol((size_t)M * cap, 0), crow((size_t)M * cap, 0);
        std::vector<double> rval((size_t)M * cap, 0.0), cval((size_t)M * cap, 0.0);
        for (int k = 0; k < M; ++k) {
            const double *g = G.data() + (size_t)k * m0 * n;
            int *rp = rptr.data() + (size_t)k * (m0 + 1), *cp = cptr.data() + (size_t)k * (n + 1);
            size_t e = 0;
            for (int i = 0; i < m0; ++i) {
                rp[i] = (int)e;
                for (int j = 0; j < n; ++j) if (g[(size_t)i * n + j] != 0.0) { rcol[(size_t)k * cap + e] = (unsigned short)j; rval[(size_t)k * cap + e] = g[(size_t)i * n + j]; ++e; }
            }
            rp[m0] = (int)e;
            e = 0;
            for (int j = 0; j < n; ++j) {
                cp[j] = (int)e;
                for (int i = 0; i < m0; ++i) if (g[(size_t)i * n + j] != 0.0) { crow[(size_t)k * cap + e] = (unsigned short)i; cval[(size_t)k * cap + e] = g[(size_t)i * n + j]; ++e; }
            }
            cp[n] = (int)e;
        }
        p->nnz_cap = (int)cap;
        if ((rc = upload(p->d_csr_ptr, rptr)) || (rc = upload(p->d_csc_ptr, cptr)) || (rc = upload(p->d_csr_col, rcol)) || (rc = upload(p->d_csc_row, crow)) ||
            (rc = upload(p->d_csr_val, rval)) || (rc = upload(p->d_csc_val, cval))) return rc;
    }
    {
        std::vector<int> pos(n, -1), perm(n);
        for (int k = 0; k < p->nb; ++k) pos[bins[k]] = k;
        // dictionary column order: position-major (all horizon steps of one per-step variable adjacent), so that the
        // non-zeros of a pivot row -- which follow the per-step coupling pattern -- fall into few 64-byte sectors
        int c = 0;
        for (int q = 0; q < p->nv; ++q) for (int k = 0; k < N_tilde; ++k) perm[c++] = k * p->nv + q;
        std::vector<double> Gp((size_t)M * m0 * n);
        for (size_t r = 0; r < (size_t)M * m0; ++r)
            for (int k = 0; k < n; ++k) Gp[r * n + k] = G[r * n + perm[k]];
        if ((rc = upload(p->d_is_int, is_int)) || (rc = upload(p->d_bins, bins)) || (rc = upload(p->d_binpos, pos)) || (rc = upload(p->d_colperm, perm)) ||
            (rc = upload(p->d_Gp, Gp))) return rc;
        hipError_t e = p->d_qs.alloc((size_t)std::max(1, n) * M);
        if (e == hipSuccess) e = p->d_q0.alloc((size_t)std::max(1, n) * M);
        if (e == hipSuccess) e = p->d_cx.alloc((size_t)std::max(1, p->nx) * M);
        if (e == hipSuccess) e = p->d_cw.alloc((size_t)std::max(1, p->nW) * M);
        if (e == hipSuccess) e = p->d_c0.alloc(M);
        if (e == hipSuccess) e = p->d_counter.alloc(1);
        if (e != hipSuccess) { mld_set_error("problem alloc: %s", hipGetErrorString(e)); return MLD_ERR_HIP; }
    }
    // 3b. LDS-resident LP path: Toeplitz-compatible equilibration (one factor per row-in-step and per variable-in-step, so that the
    //     scaled H_v is still block Toeplitz) of the tightened model's lag blocks; only time-invariant models
    if (model->tv_N == 0 && m0 && n && p->tight->d_blocks) {
        const int N = N_tilde, nc = d.nc, nv = p->nv;
        const CondLayout &L = p->tight->lay;
        std::vector<double> blk((size_t)M * N * nc * nv), rst((size_t)M * m0), cst((size_t)M * n), lbt((size_t)M * n), ubt((size_t)M * n);
        bool okc = true;
        for (int k = 0; k < M && okc; ++k)
            okc = hipMemcpy(blk.data() + (size_t)k * N * nc * nv, p->tight->d_blocks + (size_t)k * L.blk_stride + L.offV[2], sizeof(double) * N * nc * nv, hipMemcpyDeviceToHost) == hipSuccess;
        if (okc) {
            for (int k = 0; k < M; ++k) {
                double *b = blk.data() + (size_t)k * N * nc * nv;
                std::vector<double> r(nc, 1.0), c(nv, 1.0), cmax(nv);
                for (int pass = 0; pass < 3; ++pass) {
                    for (int i = 0; i < nc; ++i) {
                        double mx = 0;
                        for (int lag = 0; lag < N; ++lag) for (int j = 0; j < nv; ++j) mx = std::max(mx, std::fabs(b[((size_t)lag * nc + i) * nv + j]) * r[i] * c[j]);
                        if (mx > 0) r[i] /= mx;
                    }
                    std::fill(cmax.begin(), cmax.end(), 0.0);
                    for (int lag = 0; lag < N; ++lag) for (int i = 0; i < nc; ++i) for (int j = 0; j < nv; ++j) cmax[j] = std::max(cmax[j], std::fabs(b[((size_t)lag * nc + i) * nv + j]) * r[i] * c[j]);
                    for (int j = 0; j < nv; ++j) if (!is_int[j] && cmax[j] > 0) c[j] /= cmax[j];
                }
                for (int i = 0; i < nc; ++i) r[i] = std::exp2(std::rint(std::log2(r[i])));
                for (int j = 0; j < nv; ++j) c[j] = std::exp2(std::rint(std::log2(c[j])));
                for (int lag = 0; lag < N; ++lag) for (int i = 0; i < nc; ++i) for (int j = 0; j < nv; ++j) b[((size_t)lag * nc + i) * nv + j] *= r[i] * c[j];
                for (int i = 0; i < m0; ++i) rst[(size_t)k * m0 + i] = r[i % nc];
                for (int j = 0; j < n; ++j) { const double cj = c[j % nv]; cst[(size_t)k * n + j] = cj; lbt[(size_t)k * n + j] = lb[j] / cj; ubt[(size_t)k * n + j] = ub[j] / cj; }
            }
            LpShape &LS = p->LS;
            LS.n = n; LS.m = m0; LS.N = N; LS.nc = nc; LS.nv = nv; LS.nx = p->nx; LS.nW = p->nW; LS.max_pivots = p->opts.max_pivots;
            int dev = 0; hipDeviceProp_t prop;
            (void)hipGetDevice(&dev); (void)hipGetDeviceProperties(&prop, dev);
            const size_t budget = 160 * 1024 - 1024;      /* CDNA4: 160 KB per workgroup; static LDS of the kernel is < 1 KB */
            auto dbl_for = [&](int kc) { return (size_t)N * nc * nv + (size_t)kc * (kc + 1) + 3 * (size_t)n + m0 + 6 * (size_t)kc + (2 * ((size_t)n + m0 + 4 * (size_t)kc) + 3 * (size_t)n + m0 + 7) / 8 + 1; };   /* doubles before the fp32 bounds */
            auto lds_for = [&](int kc) { return sizeof(double) * dbl_for(kc) + sizeof(float) * 2 * (size_t)n + 64; };
            int kc = std::min(128, std::min(n, m0));
            if (p->opts.reserved & MLD_DBG_LP_LDS_K24) kc = std::min(kc, 24);      /* diagnostics: a small working-basis capacity so that the overflow fall-back runs */
            while (kc >= 8 && lds_for(kc) > budget) kc -= 4;
            if (kc >= 8 && n < 32767 && m0 < 32767) {
                LS.kcap = kc; LS.ldw = kc + 1; LS.f32_off = (int)dbl_for(kc); p->lp_lds_bytes = lds_for(kc);
                p->lp_slots = prop.multiProcessorCount;
                if ((rc = upload(p->d_blk_t, blk)) || (rc = upload(p->d_rs_t, rst)) || (rc = upload(p->d_cs_t, cst)) || (rc = upload(p->d_lb_t, lbt)) || (rc = upload(p->d_ub_t, ubt))) return rc;
                const hipError_t e = p->d_qs_t.alloc((size_t)n * M);
                if (e != hipSuccess) { mld_set_error("lp path alloc: %s", hipGetErrorString(e)); return MLD_ERR_HIP; }
                p->lp_ok = true;
            }
        }
    }
    // 4. cost (K4)
    if ((rc = set_cost_impl(p.get(), cost))) return rc;
    // 5. workspace: one dictionary per resident workgroup
    if ((rc = build_shape(p.get()))) return rc;
    {
        int dev = 0; hipDeviceProp_t prop;
        (void)hipGetDevice(&dev); (void)hipGetDeviceProperties(&prop, dev);
        if (p->lds_bytes > 48 * 1024 && p->lds_bytes <= 150 * 1024)
            (void)hipFuncSetAttribute((const void *)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds_bytes);
        int per_cu = 0;   /* resident workgroups per CU for this LDS size (the kernel's 256 VGPRs allow one): a larger grid would only queue */
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_solve, SOL_NT, p->lds_bytes) != hipSuccess || per_cu < 1) per_cu = 1;
        p->n_slots = p->opts.n_slots > 0 ? p->opts.n_slots : per_cu * prop.multiProcessorCount;
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        while (p->n_slots > 1 && (size_t)p->n_slots * p->S.ws_stride > free_b / 2) p->n_slots /= 2;
        if (p->lds_bytes > 150 * 1024) { mld_set_error("problem too large for LDS staging (%zu bytes)", p->lds_bytes); return MLD_ERR_UNSUPPORTED; }
        hipError_t e = p->d_ws.alloc((size_t)p->n_slots * p->S.ws_stride);
        if (e != hipSuccess) { mld_set_error("workspace alloc (%zu MB): %s", (size_t)p->n_slots * p->S.ws_stride >> 20, hipGetErrorString(e)); return MLD_ERR_HIP; }
        if (p->lds_bytes > 48 * 1024)
            (void)hipFuncSetAttribute((const void *)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds_bytes);
    }
    *out = p.release();
    return MLD_OK;
}

int mld_problem_set_cost(mld_problem_t *p, const mld_cost *cost)
{
    MLD_NOT_IN_FLIGHT(p, "mld_problem_set_cost");
    if (!p) { mld_set_error("null problem"); return MLD_ERR_INVALID; }
    return set_cost_impl(p, cost);
}

int mld_cost_assemble(mld_problem_t *p, double *P, double *q0, double *Qx, double *Qw)
{
    if (!p) { mld_set_error("null problem"); return MLD_ERR_INVALID; }
    const size_t n = p->n, M = p->n_models;
    if (q0) HIP_TRY(hipMemcpy(q0, p->d_q0, sizeof(double) * n * M, hipMemcpyDeviceToHost));
    if (P) { if (p->d_P) HIP_TRY(hipMemcpy(P, p->d_P, sizeof(double) * n * n * M, hipMemcpyDeviceToHost)); else memset(P, 0, sizeof(double) * n * n * M); }
    if (Qx && p->nx) { if (p->d_Qx) HIP_TRY(hipMemcpy(Qx, p->d_Qx, sizeof(double) * n * p->nx * M, hipMemcpyDeviceToHost)); else memset(Qx, 0, sizeof(double) * n * p->nx * M); }
    if (Qw && p->nW) { if (p->d_Qw) HIP_TRY(hipMemcpy(Qw, p->d_Qw, sizeof(double) * n * p->nW * M, hipMemcpyDeviceToHost)); else memset(Qw, 0, sizeof(double) * n * p->nW * M); }
    return MLD_OK;
}

/* instances grouped by model (stable counting sort) and cut into workgroup-sized chunks: the batch as the N dimension of one GEMM
 * per model.  perm is empty when the instances of every model are already contiguous in order (model_idx == NULL). */
static void build_rhs_groups(const int32_t *model_idx, int batch, int n_models, std::vector<int> &perm, std::vector<RhsGroup> &groups)
{
    perm.clear(); groups.clear();
    if (!model_idx) {
        for (int s = 0; s < batch; s += RM_NI) groups.push_back(RhsGroup{0, s, std::min(RM_NI, batch - s)});
        return;
    }
    std::vector<int> cnt(n_models + 1, 0);
    for (int b = 0; b < batch; ++b) cnt[model_idx[b] + 1]++;
    for (int k = 0; k < n_models; ++k) cnt[k + 1] += cnt[k];
    perm.resize(batch);
    std::vector<int> pos(cnt.begin(), cnt.end() - 1);
    for (int b = 0; b < batch; ++b) perm[pos[model_idx[b]]++] = b;
    for (int k = 0; k < n_models; ++k)
        for (int s = cnt[k]; s < cnt[k + 1]; s += RM_NI) groups.push_back(RhsGroup{k, s, std::min(RM_NI, cnt[k + 1] - s)});
}

static bool rhs_mfma_fits(int nx, int nW) { return ((nx + nW + 3) & ~3) <= RM_KMAX; }

static void launch_rhs_mfma(bool f32, int n_groups, int m0, int nx, int nW, const double *Hx, const double *Hw, const double *H5, const double *rs,
                            const RhsGroup *groups, const int *perm, const double *x0, const double *omega, double *hs, hipStream_t stream = 0)
{
    const int Kp = (nx + nW + 3) & ~3;
    const size_t lds = sizeof(double) * 16 * (size_t)(Kp + 1);
    if (f32) hipLaunchKernelGGL(k_rhs_mfma<true>, dim3(n_groups), dim3(64 * RM_WAVES), lds, stream, m0, nx, nW, Kp, Hx, Hw, H5, rs, groups, perm, x0, omega, hs);
    else hipLaunchKernelGGL(k_rhs_mfma<false>, dim3(n_groups), dim3(64 * RM_WAVES), lds, stream, m0, nx, nW, Kp, Hx, Hw, H5, rs, groups, perm, x0, omega, hs);
}

/* entries the per-entry arrays need for a batch: with the in-kernel hand-off the queue has room for ho_factor x batch items (at least 4096) behind the instances */
static size_t entry_cap_for(const mld_problem *p, int batch)
{
    if (!p->ho_enable) return (size_t)batch;
    return (size_t)batch + std::max<size_t>(4096, (size_t)(p->ho_factor * (double)batch));
}

static int ensure_batch(mld_problem *p, int batch)
{
    const size_t cap = entry_cap_for(p, batch);
    if (batch <= p->in_cap && cap <= (size_t)p->batch_cap) return MLD_OK;
    free_batch(p);
    const size_t b = batch;
    /* inputs: one per instance */
    HIP_TRY(p->bat.model_idx.alloc(b));
    HIP_TRY(p->bat.x0.alloc(b * std::max(1, p->nx)));
    HIP_TRY(p->bat.omega.alloc(b * std::max(1, p->nW)));
    HIP_TRY(p->bat.x0b.alloc(b * std::max(1, p->nx)));
    HIP_TRY(p->bat.omegab.alloc(b * std::max(1, p->nW)));
    HIP_TRY(p->bat.warm.alloc(b * std::max(1, p->nb)));
    HIP_TRY(p->bat.skipped.alloc(1));
    HIP_TRY(p->bat.hs.alloc(b * std::max(1, p->m0)));
    HIP_TRY(p->bat.qs_inst.alloc(b * std::max(1, p->n)));
    HIP_TRY(p->bat.rconst.alloc(b));
    HIP_TRY(p->bat.order.alloc(b));
    /* per entry (instances, then the items of the in-kernel hand-off) */
    HIP_TRY(p->bat.fixed.alloc(cap * std::max(1, p->nb)));
    HIP_TRY(p->bat.cutoff.alloc(cap));
    HIP_TRY(p->bat.open_depth.alloc(cap));
    HIP_TRY(p->bat.open_var.alloc(cap * std::max(1, p->nb)));
    HIP_TRY(p->bat.open_val.alloc(cap * std::max(1, p->nb)));
    HIP_TRY(p->bat.open_flag.alloc(cap * std::max(1, p->nb)));
    HIP_TRY(p->bat.v.alloc(cap * std::max(1, p->n)));
    HIP_TRY(p->bat.obj.alloc(cap));
    HIP_TRY(p->bat.lbnd.alloc(cap));
    HIP_TRY(p->bat.status.alloc(cap)); HIP_TRY(p->bat.nodes.alloc(cap));
    HIP_TRY(p->bat.pivots.alloc(cap)); HIP_TRY(p->bat.cuts.alloc(cap));
    HIP_TRY(p->bat.refac.alloc(cap));
    HIP_TRY(hipMemset(p->bat.status, 0, sizeof(int) * cap));      /* (ADVICE r3: a reallocation must not leave stale statuses for mld_warm_start_from_previous) */
    HIP_TRY(p->bat.ticks.alloc(cap)); HIP_TRY(p->bat.rows.alloc(cap));
    HIP_TRY(p->bat.prof.alloc(cap * 8));
    if (p->ho_enable) {
        HIP_TRY(p->bat.ho.tail.alloc(1)); HIP_TRY(p->bat.ho.finished.alloc(1));
        HIP_TRY(p->bat.ho.item_src.alloc(cap)); HIP_TRY(p->bat.ho.item_root.alloc(cap));
        HIP_TRY(p->bat.ho.item_gen.alloc(cap)); HIP_TRY(p->bat.ho.item_ready.alloc(cap));
        HIP_TRY(p->bat.ho.item_children.alloc(cap)); HIP_TRY(p->bat.ho.item_label.alloc(cap));
        HIP_TRY(p->bat.ho.mg_best.alloc(b)); HIP_TRY(p->bat.ho.mg_lbopen.alloc(b));
        HIP_TRY(p->bat.ho.mg_label.alloc(b)); HIP_TRY(p->bat.ho.mg_open.alloc(b));
        HIP_TRY(p->bat.ho.tree_count.alloc(b * 9)); HIP_TRY(p->bat.ho.tree_dead.alloc(b));
    }
    p->order_batch = 0;
    p->in_cap = batch;
    p->batch_cap = (int)cap;
    return MLD_OK;
}

int mld_upload_batch(mld_problem_t *p, int batch, const int32_t *model_idx, const double *x0, const double *omega,
                     const uint8_t *fixed_bin)
{
    MLD_NOT_IN_FLIGHT(p, "mld_upload_batch");
    if (!p || batch < 1) { mld_set_error("mld_upload_batch: bad arguments"); return MLD_ERR_INVALID; }
    if ((p->nx && !x0) || (p->nW && !omega)) { mld_set_error("mld_upload_batch: x0/omega required"); return MLD_ERR_INVALID; }
    if (model_idx) for (int b = 0; b < batch; ++b) if (model_idx[b] < 0 || model_idx[b] >= p->n_models) { mld_set_error("model_idx[%d]=%d out of range", b, model_idx[b]); return MLD_ERR_INVALID; }
    int rc = ensure_batch(p, batch);
    if (rc) { p->batch = 0; return rc; }
    p->batch = batch; p->has_midx = model_idx != nullptr; p->has_fixed = fixed_bin != nullptr;
    p->has_warm = false; p->solved = false; p->advanced = false; p->has_cutoff = false;
    p->all_fixed = false;
    if (fixed_bin && p->nb) { bool all = true; const size_t tot = (size_t)batch * p->nb; for (size_t k = 0; k < tot && all; ++k) all = fixed_bin[k] != 255; p->all_fixed = all; }
    p->n_xcols = 0;   /* extra constraint blocks belong to one upload */
    if (p->slog.cap) p->slog = mld_problem::SimLog();      /* so does a simulation log */
    if (p->ic_ld) { p->bat.icost.reset(); p->bat.qs_inst_t.reset(); p->ic_ld = 0; }   /* so does a per-instance cost */
    if (p->order_batch != batch) p->order_batch = 0;
    {
        std::vector<int> perm; std::vector<RhsGroup> groups;
        build_rhs_groups(model_idx, batch, p->n_models, perm, groups);
        p->bat.perm.reset(); p->bat.groups.reset();
        p->n_groups = (int)groups.size();
        if ((rc = upload(p->bat.perm, perm)) || (rc = upload(p->bat.groups, groups))) return rc;
    }
    if (model_idx) HIP_TRY(hipMemcpy(p->bat.model_idx, model_idx, sizeof(int) * batch, hipMemcpyHostToDevice));
    if (p->nx) HIP_TRY(hipMemcpy(p->bat.x0, x0, sizeof(double) * (size_t)batch * p->nx, hipMemcpyHostToDevice));
    if (p->nW) HIP_TRY(hipMemcpy(p->bat.omega, omega, sizeof(double) * (size_t)batch * p->nW, hipMemcpyHostToDevice));
    if (fixed_bin && p->nb) HIP_TRY(hipMemcpy(p->bat.fixed, fixed_bin, (size_t)batch * p->nb, hipMemcpyHostToDevice));
    return MLD_OK;
}

int mld_upload_constraint_blocks_x(mld_problem_t *p, int n_cols, const double *omega_cols, const int32_t *col_rows, const double *x_cols);
int mld_upload_constraint_blocks(mld_problem_t *p, int n_cols, const double *omega_cols, const int32_t *col_rows)
{
    return mld_upload_constraint_blocks_x(p, n_cols, omega_cols, col_rows, nullptr);
}

int mld_upload_constraint_blocks_x(mld_problem_t *p, int n_cols, const double *omega_cols, const int32_t *col_rows, const double *x_cols)
{
    MLD_NOT_IN_FLIGHT(p, "mld_upload_constraint_blocks");
    if (!p || p->batch < 1) { mld_set_error("mld_upload_constraint_blocks: upload the batch first"); return MLD_ERR_INVALID; }
    if (n_cols < 0 || (n_cols > 0 && p->nW && !omega_cols)) { mld_set_error("mld_upload_constraint_blocks: bad arguments"); return MLD_ERR_INVALID; }
    if (col_rows) for (int c = 0; c < n_cols; ++c) if (col_rows[c] < 0 || col_rows[c] > p->m0) { mld_set_error("col_rows[%d]=%d outside [0,%d]", c, col_rows[c], p->m0); return MLD_ERR_INVALID; }
    p->n_xcols = 0;
    if (n_cols == 0 || !p->nW) return MLD_OK;
    const size_t need = (size_t)p->batch * n_cols * p->nW;
    if (need > p->xcols_cap) {
        p->xcols_cap = 0;
        HIP_TRY(p->bat.xcols.alloc(need));
        p->xcols_cap = need;
    }
    p->bat.xrows.reset();
    HIP_TRY(hipMemcpy(p->bat.xcols, omega_cols, sizeof(double) * need, hipMemcpyHostToDevice));
    if (col_rows) {
        HIP_TRY(p->bat.xrows.alloc(n_cols));
        HIP_TRY(hipMemcpy(p->bat.xrows, col_rows, sizeof(int) * n_cols, hipMemcpyHostToDevice));
    }
    p->has_xcols_x = false;
    if (x_cols && p->nx) {
        const size_t nxs = (size_t)p->batch * n_cols * p->nx;
        HIP_TRY(p->bat.xcols_x.alloc(nxs));
        HIP_TRY(hipMemcpy(p->bat.xcols_x, x_cols, sizeof(double) * nxs, hipMemcpyHostToDevice));
        p->has_xcols_x = true;
    }
    p->n_xcols = n_cols;
    return MLD_OK;
}


// ---- in-kernel hand-off: merging the items of a tree into its root instance (after k_solve, same stream) ---------------------------------------
// order-preserving map double -> unsigned 64 (atomicMin on it = minimum of the doubles)
__device__ __forceinline__ unsigned long long mg_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double mg_val(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ bool mg_unclosed(int st) { return st == MLD_STATUS_NODE_LIMIT || st == MLD_STATUS_NUMERICAL || st == MLD_STATUS_EXPANDED_OPEN; }

__global__ void __launch_bounds__(256) k_merge_init(int batch, const double *obj, unsigned long long *best, unsigned long long *lbopen, unsigned long long *label, int *open_cnt)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= batch) return;
    best[r] = mg_key(obj[r]); lbopen[r] = mg_key(__builtin_huge_val()); label[r] = ~0ull; open_cnt[r] = 0;
}
// pass A: every item adds itself to its root -- best objective, what it left open, work counters
__global__ void __launch_bounds__(256) k_merge_a(int batch, const int *tail, const int *root, const double *obj, const double *lb, const int *status,
                                                 int *nodes, int *pivots, int *cuts, int *refac, long long *rows,
                                                 unsigned long long *best, unsigned long long *lbopen, int *open_cnt, const int *dead)
{
    const int it = batch + blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= *tail) return;
    const int r = root[it];
    if (dead[r]) return;              // a tree that was given up keeps its root's own result
    atomicMin(&best[r], mg_key(obj[it]));
    if (mg_unclosed(status[it])) { atomicAdd(&open_cnt[r], 1); atomicMin(&lbopen[r], mg_key(lb[it])); }
    atomicAdd(&nodes[r], nodes[it]); atomicAdd(&pivots[r], pivots[it]); atomicAdd(&cuts[r], cuts[it]); atomicAdd(&refac[r], refac[it]);
    atomicAdd((unsigned long long *)&rows[r], (unsigned long long)rows[it]);
}
// pass B: among the entries that hold the best objective the smallest tree label wins (deterministic whatever the queue order was)
__global__ void __launch_bounds__(256) k_merge_b(int batch, const int *tail, const int *root, const double *obj, const long long *lab,
                                                 const unsigned long long *best, unsigned long long *label, const int *dead)
{
    const int it = batch + blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= *tail) return;
    const int r = root[it];
    if (dead[r]) return;
    if (mg_key(obj[it]) == best[r] && obj[it] < 1.0e300) atomicMin(&label[r], (unsigned long long)lab[it]);
}
// pass C: the winning item's point becomes the root's (one workgroup per item; the root's own point stays when its objective is the best)
__global__ void __launch_bounds__(256) k_merge_c(int batch, const int *tail, int n, const int *root, const double *obj, const long long *lab,
                                                 const unsigned long long *best, const unsigned long long *label, double *v, const int *dead)
{
    const int it = batch + blockIdx.x;
    if (it >= *tail) return;
    const int r = root[it];
    if (dead[r]) return;
    if (mg_key(obj[it]) != best[r] || !(obj[it] < 1.0e300) || (unsigned long long)lab[it] != label[r]) return;
    if (mg_key(obj[r]) == best[r]) return;       // (the root found the same value itself: label 1 is the smallest)
    for (int j = threadIdx.x; j < n; j += blockDim.x) v[(size_t)r * n + j] = v[(size_t)it * n + j];
}
// pass D: status, objective and bound of every root that was split
__global__ void __launch_bounds__(256) k_merge_d(int batch, double gap_abs, double gap_rel, double *obj, double *lb, int *status,
                                                 const unsigned long long *best, const unsigned long long *lbopen, const int *open_cnt, int *n_unfinished, const int *dead, int *n_dead)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= batch) return;
    if (dead[r]) {                   // given up: the root's own incumbent and bound, as it stopped
        if (status[r] == MLD_STATUS_EXPANDED || status[r] == MLD_STATUS_EXPANDED_OPEN) status[r] = MLD_STATUS_NODE_LIMIT;
        atomicAdd(n_unfinished, 1); atomicAdd(n_dead, dead[r] == 2 ? 65536 : 1);
        return;
    }
    if (status[r] != MLD_STATUS_EXPANDED && status[r] != MLD_STATUS_EXPANDED_OPEN) return;
    const bool own_open = status[r] == MLD_STATUS_EXPANDED_OPEN;
    const double o = mg_val(best[r]);
    const bool fin = o < 1.0e300;
    const double tol = fin ? fmax(gap_abs, gap_rel * fabs(o)) : 0.0;
    obj[r] = o;
    if (open_cnt[r] == 0 && !own_open) {       // every node of the tree is closed: proven
        status[r] = fin ? MLD_STATUS_OPTIMAL : MLD_STATUS_INFEASIBLE;
        if (fin) lb[r] = fmin(o, fmax(lb[r], o - tol));
    } else {
        status[r] = MLD_STATUS_NODE_LIMIT;
        lb[r] = own_open ? fmin(lb[r], fin ? o : __builtin_huge_val())      /* (the root's own rest is open: its bound, valid for the whole tree, stands) */
                         : fmax(lb[r], fmin(mg_val(lbopen[r]), fin ? o - tol : __builtin_huge_val()));
        atomicAdd(n_unfinished, 1);
    }
}
__global__ void k_set_int(int *dst, int value) { *dst = value; }
__global__ void k_fill_f64(size_t count, double value, double *out)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) out[k] = value;
}

// per-batch solver statistics reduced on the device: one 64-byte copy instead of five batch-sized ones (the small-batch latency is host overhead)
__global__ void __launch_bounds__(256) k_batch_stats(int batch, const int *status, const int *nodes, const int *pivots, const int *cuts, const int *refac, long long *out)
{
    __shared__ long long acc[8];
    if (threadIdx.x < 8) acc[threadIdx.x] = 0;
    __syncthreads();
    long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < batch; i += 256) {
        v[0] += nodes[i]; v[1] += pivots[i]; v[2] += cuts[i]; v[3] += refac[i];
        const int s = status[i];
        if (s == MLD_STATUS_OPTIMAL) v[4]++; else if (s == MLD_STATUS_INFEASIBLE) v[5]++; else if (s == MLD_STATUS_NODE_LIMIT) v[6]++; else v[7]++;
    }
    for (int q = 0; q < 8; ++q) if (v[q]) atomicAdd((unsigned long long *)&acc[q], (unsigned long long)v[q]);
    __syncthreads();
    if (threadIdx.x < 8) out[threadIdx.x] = acc[threadIdx.x];
}

/* the per-instance linear cost of the resident batch as the solve kernels read it, at the CURRENT inputs (staged / advanced ones included):
 * qs_inst = cs (q0 + q_b) -- under a quadratic cost k_qinst has written it with the Qx x0 + Qw omega term already -- and rconst (+)= the
 * constant cx_b' x0 + cw_b' omega + c0_b.  lds: also the copy under the Toeplitz-compatible column scales (k_lp_lds). */
static int launch_inst_cost(mld_problem *p, bool lds)
{
    const hipStream_t sq = p->stream;
    const int batch = p->batch, n = p->n;
    const size_t tot = (size_t)batch * n;
    if (!p->has_quad) {
        if (tot) hipLaunchKernelGGL(k_inst_cost, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, sq, tot, n, p->ic_ld, p->d_q0, p->d_cs, lds ? p->d_cs_t.get() : nullptr,
                                    p->has_midx ? p->bat.model_idx.get() : nullptr, p->bat.icost, p->bat.qs_inst, lds ? p->bat.qs_inst_t.get() : nullptr);
        HIP_TRY(hipMemsetAsync(p->bat.rconst, 0, sizeof(double) * batch, sq));
    }
    if (p->ic_ld > n)
        hipLaunchKernelGGL(k_inst_const, dim3((batch + 3) / 4), dim3(256), 0, sq, batch, n, p->nx, p->nW, p->ic_ld, p->bat.icost, p->bat.x0, p->bat.omega, p->bat.rconst);
    return MLD_OK;
}

/* LDS-resident LP path -- relaxation-only mode: every binary fixed -> one LP per instance, solved in LDS (k_lp_lds); right-hand sides with the
 * Toeplitz row scales.  Runs to completion: redo lists the instances whose working basis outgrew LDS (status -1), for the dense kernel. */
static int launch_lds_lp(mld_problem *p, std::vector<int> &redo)
{
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    const mld_model *t = p->tight.get();
    launch_rhs_mfma((p->opts.flags & MLD_F32) != 0, p->n_groups, p->m0, p->nx, p->nW, t->d_out[O_HX], t->d_out[O_HW], t->d_out[O_H5], p->d_rs_t,
                    p->bat.groups, p->bat.perm, p->bat.x0, p->bat.omega, p->bat.hs, sq);
    if (p->n_xcols > 0)
        hipLaunchKernelGGL(k_rhs_extra, dim3(batch), dim3(256), 0, sq, p->m0, p->nx, p->nW, t->d_out[O_HX], t->d_out[O_HW], t->d_out[O_H5],
                           p->d_rs_t, p->has_midx ? p->bat.model_idx.get() : nullptr, p->bat.x0, p->bat.xcols, p->n_xcols, p->bat.xrows, p->bat.hs, p->has_xcols_x ? p->bat.xcols_x.get() : nullptr);
    if (p->ic_ld) {      /* per-instance cost under the Toeplitz-compatible column scales, and its constant at the current inputs */
        if (!p->bat.qs_inst_t) HIP_TRY(p->bat.qs_inst_t.alloc((size_t)batch * std::max(1, p->n)));
        if (int rc = launch_inst_cost(p, true)) return rc;
    }
    HIP_TRY(hipEventRecord(p->ev[1], sq));
    LpModelDev LM; LM.blk = p->d_blk_t; LM.qs = p->d_qs_t; LM.lb = p->d_lb_t; LM.ub = p->d_ub_t; LM.cs = p->d_cs_t;
    LM.cx = p->nx ? p->d_cx.get() : nullptr; LM.cw = p->nW ? p->d_cw.get() : nullptr; LM.c0 = p->d_c0; LM.bins = p->d_bins; LM.nb = p->nb; LM.is_int = p->d_is_int;
    LpBatchDev LB; LB.batch = batch; LB.model_idx = p->has_midx ? p->bat.model_idx.get() : nullptr; LB.x0 = p->bat.x0; LB.omega = p->bat.omega; LB.hs = p->bat.hs;
    LB.fixed = p->bat.fixed; LB.v_out = p->bat.v; LB.obj_out = p->bat.obj; LB.lb_out = p->bat.lbnd; LB.status_out = p->bat.status; LB.nodes_out = p->bat.nodes;
    LB.pivots_out = p->bat.pivots; LB.ticks_out = p->bat.ticks; LB.prof_out = p->bat.prof; LB.counter = p->d_counter; LB.cuts_out = p->bat.cuts;
    LB.qs_inst = p->ic_ld ? p->bat.qs_inst_t.get() : nullptr; LB.rconst = p->ic_ld ? p->bat.rconst.get() : nullptr;
    p->LS.max_pivots = p->opts.max_pivots;
    HIP_TRY(hipMemsetAsync(p->bat.cuts, 0, sizeof(int) * batch, sq));
    HIP_TRY(hipFuncSetAttribute((const void *)k_lp_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lp_lds_bytes));
    hipLaunchKernelGGL(k_lp_lds, dim3(std::min(batch, p->lp_slots)), dim3(LP_NT), p->lp_lds_bytes, sq, p->LS, LM, LB, (unsigned char *)nullptr);
    HIP_TRY(hipMemsetAsync(p->bat.refac, 0, sizeof(int) * batch, sq));
    HIP_TRY(hipMemsetAsync(p->bat.rows, 0, sizeof(long long) * batch, sq));
    HIP_TRY(hipStreamSynchronize(sq));
    HIP_TRY(hipGetLastError());
    std::vector<int> stat(batch);
    HIP_TRY(hipMemcpy(stat.data(), p->bat.status, sizeof(int) * batch, hipMemcpyDeviceToHost));
    redo.clear();
    if (!(p->opts.reserved & MLD_DBG_LP_LDS_NO_REDO))      /* diagnostics: leave status -1 visible instead of re-solving */
        for (int i = 0; i < batch; ++i) if (stat[i] == -1) redo.push_back(i);
    return MLD_OK;
}

/* right-hand sides of the dense path (K3) with the extra constraint blocks, and the per-instance part of the cost (quadratic atoms, mld_upload_instance_cost) */
static int launch_rhs_cost(mld_problem *p)
{
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    const mld_model *t = p->tight.get();
    const int *midx = p->has_midx ? p->bat.model_idx.get() : nullptr;
    if (p->m0 && !p->std_block)        /* no standard block: every row starts without a right-hand side; the extra blocks' row-wise minimum follows */
        hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)(((size_t)batch * p->m0 + 255) / 256)), dim3(256), 0, sq, (size_t)batch * p->m0, 1.0e30, p->bat.hs);
    else if (p->m0 && rhs_mfma_fits(p->nx, p->nW) && !(p->opts.reserved & MLD_DBG_GEMM_VALU))     /* K3 as one GEMM per model on the matrix cores */
        launch_rhs_mfma((p->opts.flags & MLD_F32) != 0, p->n_groups, p->m0, p->nx, p->nW, t->d_out[O_HX], t->d_out[O_HW], t->d_out[O_H5], p->d_rs,
                        p->bat.groups, p->bat.perm, p->bat.x0, p->bat.omega, p->bat.hs, sq);
    else if (p->m0)
        hipLaunchKernelGGL(k_rhs, dim3(batch), dim3(256), 0, sq, p->m0, p->nx, p->nW, t->d_out[O_HX], t->d_out[O_HW], t->d_out[O_H5],
                           p->d_rs, midx, p->bat.x0, p->bat.omega, p->bat.hs, 1);
    if (p->m0 && p->n_xcols > 0)
        hipLaunchKernelGGL(k_rhs_extra, dim3(batch), dim3(256), 0, sq, p->m0, p->nx, p->nW, t->d_out[O_HX], t->d_out[O_HW], t->d_out[O_H5],
                           p->d_rs, midx, p->bat.x0, p->bat.xcols, p->n_xcols, p->bat.xrows, p->bat.hs, p->has_xcols_x ? p->bat.xcols_x.get() : nullptr);
    if (p->has_quad) {
        const int NX = p->N * p->model->dims.nx, NY = p->N * p->model->dims.ny;
        hipLaunchKernelGGL(k_qinst, dim3(batch), dim3(256), 0, sq, p->n, p->nx, p->nW, p->d_q0, p->d_Qx, p->d_Qw, p->d_cs, midx, p->bat.x0, p->bat.omega, p->bat.qs_inst,
                           p->ic_ld ? p->bat.icost.get() : nullptr, p->ic_ld);
        HIP_TRY(hipMemsetAsync(p->bat.rconst, 0, sizeof(double) * batch, sq));
        if (p->d_Wx && NX) hipLaunchKernelGGL(k_quad_const, dim3(batch), dim3(256), sizeof(double) * NX, sq, NX, p->nx, p->nW, t->d_out[O_PhiX], t->lay.out_size[O_PhiX],
                                              t->d_out[O_GamW], t->lay.out_size[O_GamW], t->d_out[O_Gam5], t->lay.out_size[O_Gam5], p->d_Wx, midx, p->bat.x0, p->bat.omega, p->bat.rconst);
        if (p->d_Wy && NY) hipLaunchKernelGGL(k_quad_const, dim3(batch), dim3(256), sizeof(double) * NY, sq, NY, p->nx, p->nW, t->d_out[O_LX], t->lay.out_size[O_LX],
                                              t->d_out[O_LW], t->lay.out_size[O_LW], t->d_out[O_L5], t->lay.out_size[O_L5], p->d_Wy, midx, p->bat.x0, p->bat.omega, p->bat.rconst);
    }
    if (p->ic_ld) return launch_inst_cost(p, false);
    return MLD_OK;
}

static ProblemDev problem_dev(const mld_problem *p)
{
    const mld_model *t = p->tight.get();
    ProblemDev P;
    P.Gp = p->d_Gp; P.Gs = p->d_Gs; P.rs = p->d_rs; P.cs = p->d_cs; P.qs = p->d_qs; P.lb = p->d_lb; P.ub = p->d_ub; P.is_int = p->d_is_int;
    P.bins = p->d_bins; P.colperm = p->d_colperm; P.Hx = t->d_out[O_HX]; P.Hw = t->d_out[O_HW]; P.H5 = t->d_out[O_H5];
    P.cx = p->nx ? p->d_cx.get() : nullptr; P.cw = p->nW ? p->d_cw.get() : nullptr; P.c0 = p->d_c0;
    P.Ps = p->has_quad ? p->d_Ps.get() : nullptr;
    P.act_max = p->d_actmax;
    P.csr_ptr = p->d_csr_ptr; P.csr_col = p->d_csr_col; P.csr_val = p->d_csr_val; P.csc_ptr = p->d_csc_ptr; P.csc_row = p->d_csc_row; P.csc_val = p->d_csc_val; P.nnz_cap = p->nnz_cap;
    P.binpos = p->d_binpos;
    return P;
}

/* the resident batch as k_solve sees it; with the in-kernel hand-off (ho) the fixings and cutoffs become per-entry arrays the items write */
static BatchDev batch_dev(const mld_problem *p, bool ho)
{
    const BatchBufs &b = p->bat;
    BatchDev B;
    B.batch = p->batch; B.model_idx = p->has_midx ? b.model_idx.get() : nullptr; B.x0 = b.x0; B.omega = b.omega;
    B.fixed = p->has_fixed || ho ? b.fixed.get() : nullptr; B.hs = b.hs;
    B.warm = p->has_warm ? b.warm.get() : nullptr;
    B.cutoff = p->has_cutoff || ho ? b.cutoff.get() : nullptr;
    B.open_depth = p->want_open ? b.open_depth.get() : nullptr; B.open_var = b.open_var; B.open_val = b.open_val; B.open_flag = b.open_flag;
    const bool inst_q = p->has_quad || p->ic_ld;      /* k_solve takes the QP relaxation on S.qp && P.Ps, never on qs_inst being there */
    B.qs_inst = inst_q ? b.qs_inst.get() : nullptr; B.rconst = inst_q ? b.rconst.get() : nullptr; B.v_out = b.v; B.obj_out = b.obj; B.lb_out = b.lbnd;
    B.status_out = b.status; B.nodes_out = b.nodes; B.pivots_out = b.pivots; B.cuts_out = b.cuts; B.refac_out = b.refac;
    B.ticks_out = b.ticks; B.rows_out = b.rows; B.prof_out = b.prof; B.trace = p->d_trace;
    B.counter = p->d_counter;
    B.order = (p->order_batch == p->batch && !(p->opts.reserved & MLD_DBG_NO_ORDER)) ? b.order.get() : nullptr;
    B.ho = ho ? 1 | (p->has_fixed ? 0 : 2) : 0; B.cap = p->batch_cap; B.tail = b.ho.tail; B.finished = b.ho.finished;
    B.ho_sub_nodes = p->ho_sub_nodes > 0 ? p->ho_sub_nodes : p->opts.max_nodes; B.ho_max_gen = p->ho_max_gen; B.ho_max_children = p->ho_max_children;
    B.item_src = b.ho.item_src; B.item_root = b.ho.item_root; B.item_gen = b.ho.item_gen; B.item_label = b.ho.item_label; B.item_ready = b.ho.item_ready;
    B.item_children = b.ho.item_children;
    B.tree_count = b.ho.tree_count; B.tree_dead = b.ho.tree_dead; B.ho_max_tree = p->ho_max_tree; B.ho_donate = p->ho_donate; B.ho_rounds = p->ho_rounds;
    return B;
}

/* an empty hand-off queue behind the batch's instances (before k_solve) */
static int handoff_reset(mld_problem *p)
{
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    const BatchBufs::Handoff &q = p->bat.ho;
    HIP_TRY(hipMemsetAsync(q.tree_count, 0, sizeof(int) * (size_t)batch * 9, sq));
    HIP_TRY(hipMemsetAsync(q.tree_dead, 0, sizeof(int) * (size_t)batch, sq));
    hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, sq, q.tail, batch);
    HIP_TRY(hipMemsetAsync(q.finished, 0, sizeof(int), sq));
    HIP_TRY(hipMemsetAsync(q.item_ready, 0, sizeof(int) * (size_t)p->batch_cap, sq));
    HIP_TRY(hipMemsetAsync(q.item_children, 0, sizeof(int) * (size_t)p->batch_cap, sq));
    if (!p->has_cutoff) hipLaunchKernelGGL(k_fill_f64, dim3((batch + 255) / 256), dim3(256), 0, sq, (size_t)batch, (double)INFINITY, p->bat.cutoff);
    return MLD_OK;
}

/* what the merge works on: the per-entry result arrays (cap entries: batch roots, then the items), the items' roots and tree labels, the
 * give-up marks and the accumulators per root, and the two device counters it reports through.  The solve path fills it from the resident batch
 * (merge_args), mld_debug_merge from arrays of the caller's. */
struct MergeArgs {
    int batch, cap, n; double gap_abs, gap_rel;
    double *obj, *lbnd, *v; int *status, *nodes, *pivots, *cuts, *refac; long long *rows;
    const int *tail, *item_root; const long long *item_label; const int *tree_dead;
    unsigned long long *mg_best, *mg_lbopen, *mg_label; int *mg_open;
    int *n_unfinished, *n_dead;      /* n_dead: + 1 per tree given up for its size, + 65536 per tree given up because the queue was full */
};

static MergeArgs merge_args(const mld_problem *p)
{
    const BatchBufs &b = p->bat;
    const BatchBufs::Handoff &q = b.ho;
    MergeArgs a;
    a.batch = p->batch; a.cap = p->batch_cap; a.n = p->n; a.gap_abs = p->opts.gap_abs; a.gap_rel = p->opts.gap_rel;
    a.obj = b.obj; a.lbnd = b.lbnd; a.v = b.v; a.status = b.status; a.nodes = b.nodes; a.pivots = b.pivots; a.cuts = b.cuts; a.refac = b.refac; a.rows = b.rows;
    a.tail = q.tail; a.item_root = q.item_root; a.item_label = q.item_label; a.tree_dead = q.tree_dead;
    a.mg_best = q.mg_best; a.mg_lbopen = q.mg_lbopen; a.mg_label = q.mg_label; a.mg_open = q.mg_open;
    a.n_unfinished = b.skipped; a.n_dead = q.finished;      /* (finished: the queue is drained, the counter is free) */
    return a;
}

/* merge the items into their roots after k_solve (deterministic: best objective, smallest tree label on ties) */
static int handoff_merge(const MergeArgs &a, hipStream_t sq)
{
    const int batch = a.batch;
    const int items = a.cap - batch;
    const dim3 gi((items + 255) / 256), gb((batch + 255) / 256), blk(256);
    HIP_TRY(hipMemsetAsync(a.n_unfinished, 0, sizeof(int), sq));
    hipLaunchKernelGGL(k_merge_init, gb, blk, 0, sq, batch, a.obj, a.mg_best, a.mg_lbopen, a.mg_label, a.mg_open);
    hipLaunchKernelGGL(k_merge_a, gi, blk, 0, sq, batch, a.tail, a.item_root, a.obj, a.lbnd, a.status, a.nodes, a.pivots, a.cuts, a.refac, a.rows,
                       a.mg_best, a.mg_lbopen, a.mg_open, a.tree_dead);
    hipLaunchKernelGGL(k_merge_b, gi, blk, 0, sq, batch, a.tail, a.item_root, a.obj, a.item_label, a.mg_best, a.mg_label, a.tree_dead);
    hipLaunchKernelGGL(k_merge_c, dim3(items), blk, 0, sq, batch, a.tail, a.n, a.item_root, a.obj, a.item_label, a.mg_best, a.mg_label, a.v, a.tree_dead);
    hipLaunchKernelGGL(k_merge_d, gb, blk, 0, sq, batch, a.gap_abs, a.gap_rel, a.obj, a.lbnd, a.status, a.mg_best, a.mg_lbopen, a.mg_open, a.n_unfinished, a.tree_dead, a.n_dead);
    return MLD_OK;
}

/* wait for the launched solve; the handle is unlocked whatever the outcome (every entry point refuses a problem that is in flight) */
static int wait_solve(mld_problem *p)
{
    const hipError_t ew = hipEventSynchronize(p->ev[2]);
    p->flight = Flight::idle;
    if (ew != hipSuccess) { mld_set_error("mld_solve: %s", hipGetErrorString(ew)); return MLD_ERR_HIP; }
    HIP_TRY(hipGetLastError());
    p->solved = true; p->advanced = false;
    return MLD_OK;
}

/* queue a solve of the resident batch on the problem's stream.  The dense path returns with k_solve queued (Flight::queued); the LDS path,
 * whose fall-back needs the statuses on the host, returns complete (Flight::lds_done) */
static int launch(mld_problem *p)
{
    if (!p || p->batch < 1) { mld_set_error("mld_solve_resident: nothing uploaded"); return MLD_ERR_INVALID; }
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    if (!p->ev_ok) {      /* the three timing events and the statistics buffer live as long as the problem */
        HIP_TRY(hipEventCreate(&p->ev[0])); HIP_TRY(hipEventCreate(&p->ev[1])); HIP_TRY(hipEventCreate(&p->ev[2]));
        HIP_TRY(p->d_statbuf.alloc(8));
        p->ev_ok = true;
    }
    if (p->flight != Flight::idle) { mld_set_error("mld_solve_launch: the previous launch has not been finished"); return MLD_ERR_INVALID; }
    HIP_TRY(hipMemsetAsync(p->d_counter, 0, sizeof(int), sq));
    HIP_TRY(hipEventRecord(p->ev[0], sq));
    const bool lp_path = p->lp_ok && p->all_fixed && !(p->opts.reserved & MLD_DBG_NO_LP_LDS) && p->std_block && !p->has_quad && rhs_mfma_fits(p->nx, p->nW);
    std::vector<int> redo;      /* LP path: the overflow instances, re-solved by k_solve */
    int rc;
    if (lp_path && (rc = launch_lds_lp(p, redo))) return rc;
    if (lp_path && redo.empty()) {
        HIP_TRY(hipEventRecord(p->ev[2], sq));
    } else {
        if (lp_path) HIP_TRY(hipMemsetAsync(p->d_counter, 0, sizeof(int), sq));
        if ((rc = launch_rhs_cost(p))) return rc;
        if (!lp_path) HIP_TRY(hipEventRecord(p->ev[1], sq));
        p->S.qp = p->has_quad ? 1 : 0;
        const bool ho = p->ho_enable && p->bat.ho.tail && !lp_path && p->nb > 0;      /* (a quadratic cost included: items index qs_inst / rconst by their source instance, < batch) */
        const ProblemDev P = problem_dev(p);
        BatchDev B = batch_dev(p, ho);
        if (ho && (rc = handoff_reset(p))) return rc;
        if (lp_path) {      /* only the overflow instances of the LP path */
            HIP_TRY(hipMemcpy(p->bat.order, redo.data(), sizeof(int) * redo.size(), hipMemcpyHostToDevice));
            p->order_batch = 0;
            B.order = p->bat.order; B.batch = (int)redo.size();
        }
        const int grid = ho ? p->n_slots : std::min(B.batch, p->n_slots);      /* (hand-off: the workgroups without an instance wait for items) */
        if (p->lds_bytes > 48 * 1024)   /* per-function limit: set for THIS problem (several problems of different size may be alive) */
            HIP_TRY(hipFuncSetAttribute((const void *)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds_bytes));
        hipLaunchKernelGGL(k_solve, dim3(grid), dim3(SOL_NT), p->lds_bytes, sq, p->S, P, B, p->d_ws.get());
        if (ho && (rc = handoff_merge(merge_args(p), sq))) return rc;
        p->ho_ran = ho;
        HIP_TRY(hipEventRecord(p->ev[2], sq));
    }
    if (!lp_path) { p->flight = Flight::queued; return MLD_OK; }
    if ((rc = wait_solve(p))) return rc;
    p->flight = Flight::lds_done;      /* (mld_solve_finish only reports -- the handle stays in flight until then, like a queued dense solve) */
    return MLD_OK;
}

/* wait for the launched solve and report: queue statistics, mld_stats, and the longest-first order for the next solve of this batch size */
static int finish(mld_problem *p, mld_stats *st)
{
    if (!p || p->batch < 1) { mld_set_error("mld_solve_resident: nothing uploaded"); return MLD_ERR_INVALID; }
    if (p->flight == Flight::idle) { mld_set_error("mld_solve_finish: no launched solve"); return MLD_ERR_INVALID; }
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    const bool dense = p->flight == Flight::queued;
    int rc;
    if ((rc = wait_solve(p))) return rc;
    if (dense && p->ho_ran) {      /* queue statistics of the launch that just ended */
        int tl = 0, unf = 0, fin = 0;
        HIP_TRY(hipMemcpyAsync(&tl, p->bat.ho.tail, sizeof(int), hipMemcpyDeviceToHost, sq));
        HIP_TRY(hipMemcpyAsync(&unf, p->bat.skipped, sizeof(int), hipMemcpyDeviceToHost, sq));
        HIP_TRY(hipMemcpyAsync(&fin, p->bat.ho.finished, sizeof(int), hipMemcpyDeviceToHost, sq));
        HIP_TRY(hipStreamSynchronize(sq));
        /* finished ended at tail and then took: + 1 per tree given up for its size, + 65536 per tree given up because the queue was full */
        const int extra = fin - tl;
        p->ho_stats[0] = tl - batch; p->ho_stats[1] = extra % 65536; p->ho_stats[2] = unf; p->ho_stats[3] = extra / 65536;
    }
    if (st) {
        memset(st, 0, sizeof(*st));
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, p->ev[0], p->ev[1])); HIP_TRY(hipEventElapsedTime(&b, p->ev[1], p->ev[2]));
        st->rhs_ms = a; st->solve_ms = b;
        long long h[8];
        hipLaunchKernelGGL(k_batch_stats, dim3(1), dim3(256), 0, sq, batch, p->bat.status, p->bat.nodes, p->bat.pivots, p->bat.cuts, p->bat.refac, p->d_statbuf);
        HIP_TRY(hipMemcpyAsync(h, p->d_statbuf, sizeof(h), hipMemcpyDeviceToHost, sq));
        HIP_TRY(hipStreamSynchronize(sq));
        st->nodes = h[0]; st->pivots = h[1]; st->cuts = h[2]; st->refactors = h[3];
        st->n_optimal = (int)h[4]; st->n_infeasible = (int)h[5]; st->n_node_limit = (int)h[6]; st->n_numerical = (int)h[7];
    }
    if (dense && batch > p->n_slots && !(p->opts.reserved & MLD_DBG_NO_ORDER)) {
        /* Work-queue order for the next solve of this batch size: longest first (LPT).  Consecutive MPC steps solve
         * nearly the same instances, so the previous in-kernel time predicts the next one; starting the long
         * branch-and-bound runs first removes the partially idle tail of the persistent grid.  Results do not depend
         * on the order (every instance is solved by one workgroup, bit-reproducibly). */
        std::vector<long long> ticks(batch);
        HIP_TRY(hipMemcpy(ticks.data(), p->bat.ticks, sizeof(long long) * batch, hipMemcpyDeviceToHost));
        std::vector<int> ord(batch);
        for (int i = 0; i < batch; ++i) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return ticks[a] > ticks[b]; });
        HIP_TRY(hipMemcpy(p->bat.order, ord.data(), sizeof(int) * batch, hipMemcpyHostToDevice));
        p->order_batch = batch;
    }
    return MLD_OK;
}

int mld_solve_resident(mld_problem_t *p, mld_stats *st)
{
    const int rc = launch(p);
    return rc ? rc : finish(p, st);
}

/* The same solve in two halves, for callers that keep several problems busy: with mld_problem_use_stream every problem owns a HIP stream, a
 * launched solve of one problem runs while another is being prepared or finished, and the workgroups of the next launch move onto the
 * CUs as the stragglers of the previous one retire (bench.py: consecutive, independent scenario sets on two problems). */
int mld_solve_launch(mld_problem_t *p) { return launch(p); }
int mld_solve_finish(mld_problem_t *p, mld_stats *st) { return finish(p, st); }
int mld_problem_use_stream(mld_problem_t *p)
{
    if (!p) { mld_set_error("mld_problem_use_stream: bad handle"); return MLD_ERR_INVALID; }
    if (p->flight != Flight::idle) { mld_set_error("mld_problem_use_stream: a solve is in flight"); return MLD_ERR_INVALID; }
    if (!p->own_stream) { HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking)); p->own_stream = true; }
    return MLD_OK;
}

int mld_download_results(mld_problem_t *p, double *v_out, double *obj_out, int32_t *status_out, double *lower_bound_out,
                         int32_t *nodes_out, int32_t *pivots_out)
{
    MLD_NOT_IN_FLIGHT(p, "mld_download_results");
    if (!p || p->batch < 1) { mld_set_error("mld_download_results: nothing solved"); return MLD_ERR_INVALID; }
    const size_t b = p->batch;
    if (v_out && p->n) HIP_TRY(hipMemcpy(v_out, p->bat.v, sizeof(double) * b * p->n, hipMemcpyDeviceToHost));
    if (obj_out) HIP_TRY(hipMemcpy(obj_out, p->bat.obj, sizeof(double) * b, hipMemcpyDeviceToHost));
    if (status_out) HIP_TRY(hipMemcpy(status_out, p->bat.status, sizeof(int) * b, hipMemcpyDeviceToHost));
    if (lower_bound_out) HIP_TRY(hipMemcpy(lower_bound_out, p->bat.lbnd, sizeof(double) * b, hipMemcpyDeviceToHost));
    if (nodes_out) HIP_TRY(hipMemcpy(nodes_out, p->bat.nodes, sizeof(int) * b, hipMemcpyDeviceToHost));
    if (pivots_out) HIP_TRY(hipMemcpy(pivots_out, p->bat.pivots, sizeof(int) * b, hipMemcpyDeviceToHost));
    return MLD_OK;
}

int mld_download_telemetry(mld_problem_t *p, int64_t *latency_ns, int64_t *rows_updated, int64_t *row_bytes)
{
    MLD_NOT_IN_FLIGHT(p, "mld_download_telemetry");
    if (!p || p->batch < 1) { mld_set_error("mld_download_telemetry: nothing solved"); return MLD_ERR_INVALID; }
    const size_t b = p->batch;
    if (latency_ns) {
        std::vector<long long> t(b);
        HIP_TRY(hipMemcpy(t.data(), p->bat.ticks, sizeof(long long) * b, hipMemcpyDeviceToHost));
        int dev = 0, khz = 100000;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
        for (size_t i = 0; i < b; ++i) latency_ns[i] = (int64_t)((double)t[i] * 1.0e6 / (double)khz);
    }
    if (rows_updated) HIP_TRY(hipMemcpy(rows_updated, p->bat.rows, sizeof(long long) * b, hipMemcpyDeviceToHost));
    if (row_bytes) *row_bytes = 8 * SOL_SEC;   /* rows_updated counts update sectors (SOL_SEC doubles) */
    return MLD_OK;
}

/* Post-mortem diagnostics (internal; not part of the public header): every resident workgroup of k_solve writes the instance it is working on and a stage code
 * into 16 ints of HOST memory that is a shared mapping of `path` -- the file survives a GPU fault that takes the process down.  Slot layout per workgroup:
 * [0] instance, [1] stage (1 start, 2 root LP, 10+r / 30+r / 50+r cut round r: Gomory / c-MIR / re-solve, 70 cut loop done, 100 + 10 phase + pass,
 * 400+ leaf, 5000+ flips of the long-step ratio test, 999 instance done), [2] pivots so far, [3] queue position.  path = NULL switches it off. */
int mld_debug_trace(mld_problem_t *p, const char *path)
{
    if (!p) return MLD_ERR_INVALID;
    if (p->h_trace) { (void)hipHostUnregister(p->h_trace); munmap(p->h_trace, p->trace_bytes); p->h_trace = nullptr; p->d_trace = nullptr; }
    if (!path) return MLD_OK;
    const size_t bytes = (size_t)std::max(1, p->n_slots) * 16 * sizeof(int);
    const int fd = open(path, O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (fd < 0 || ftruncate(fd, (off_t)bytes) != 0) { if (fd >= 0) close(fd); mld_set_error("mld_debug_trace: cannot create %s", path); return MLD_ERR_INVALID; }
    void *h = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (h == MAP_FAILED) { mld_set_error("mld_debug_trace: mmap failed"); return MLD_ERR_INVALID; }
    memset(h, 0xff, bytes);
    void *d = nullptr;
    if (hipHostRegister(h, bytes, hipHostRegisterMapped) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        munmap(h, bytes); mld_set_error("mld_debug_trace: hipHostRegister failed"); return MLD_ERR_HIP;
    }
    p->h_trace = h; p->d_trace = (int *)d; p->trace_bytes = bytes;
    return MLD_OK;
}

/* ticks per category summed over the batch (internal diagnostics; not part of the public header) */
int mld_debug_profile(mld_problem_t *p, int64_t out[8])
{
    if (!p || p->batch < 1) return MLD_ERR_INVALID;
    std::vector<long long> t((size_t)p->batch * 8);
    HIP_TRY(hipMemcpy(t.data(), p->bat.prof, sizeof(long long) * t.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; ++k) out[k] = 0;
    for (size_t i = 0; i < (size_t)p->batch; ++i) for (int k = 0; k < 8; ++k) out[k] += t[i * 8 + k];
    return MLD_OK;
}

/* the solver's shape (internal diagnostics; not part of the public header): [0..7] n, m0, mcap, first_cap, ld, mir_cap, lds_bytes, ws_stride;
 * [8..19] the LDS byte offsets (-1: in the slot) lXB, lBasic, lSkip, lAtUp, lNonbasic, lXN, lLo, lHi, lDw, lCost, lMirLine, lMirCache;
 * [20] the LDS budget of the hot arrays, [21] the MLD_SOL_SLOT mask (bit k: SLOT_NAMES[k]), [22] n_slots,
 * [23] lPair: the LDS byte offset of the second pivot's buffers of a fused pair (over lMirCache), or -1: every pivot updates on its own */
int mld_debug_shape(mld_problem_t *p, int64_t out[24])
{
    if (!p || !out) { mld_set_error("mld_debug_shape: bad arguments"); return MLD_ERR_INVALID; }
    const SolverShape &S = p->S;
    const int64_t v[24] = {S.n, S.m0, S.mcap, S.first_cap, S.ld, S.mir_cap, (int64_t)p->lds_bytes, (int64_t)S.ws_stride,
                           S.lXB, S.lBasic, S.lSkip, S.lAtUp, S.lNonbasic, S.lXN, S.lLo, S.lHi, S.lDw, S.lCost, S.lMirLine, S.lMirCache,
                           (int64_t)SOL_LDS_BUDGET, (int64_t)p->slot_mask, p->n_slots, S.lPair};
    for (int k = 0; k < 24; ++k) out[k] = v[k];
    return MLD_OK;
}

/* the MIP start of the resident batch as the next solve would read it (internal diagnostics; not part of the public header): out = batch x n_bin bytes
 * (untouched when there is no start or no binary), *has_warm = 1 when a start is set */
int mld_debug_warm_start(mld_problem_t *p, uint8_t *out, int *has_warm)
{
    MLD_NOT_IN_FLIGHT(p, "mld_debug_warm_start");
    if (!p || p->batch < 1 || !has_warm) { mld_set_error("mld_debug_warm_start: bad arguments / nothing uploaded"); return MLD_ERR_INVALID; }
    *has_warm = p->has_warm ? 1 : 0;
    if (out && p->has_warm && p->nb) HIP_TRY(hipMemcpy(out, p->bat.warm, (size_t)p->batch * p->nb, hipMemcpyDeviceToHost));
    return MLD_OK;
}

/* The hand-off merge on a queue of the caller's (internal diagnostics and tests; not part of the public header): per-entry arrays of `cap` entries -- `batch`
 * roots, then items up to `tail` -- are uploaded, handoff_merge runs on them exactly as after k_solve, and the roots' results come back in place
 * (obj, lbnd, status, nodes, pivots, cuts, refac, rows: entries < batch; v: rows < batch of cap x n).  item_root / item_label: cap entries, read in
 * [batch, tail); tree_dead: batch entries (0, 1 = given up for its size, 2 = for a full queue).  n_unfinished, finished: the two device counters, finished
 * starting at tail as a drained queue leaves it.  Everything a kernel indexes with is validated here. */
struct mld_debug_merge_io {
    int32_t batch, cap, n, tail; double gap_abs, gap_rel;
    double *obj, *lbnd, *v; int32_t *status, *nodes, *pivots, *cuts, *refac; int64_t *rows;
    const int32_t *item_root; const int64_t *item_label; const int32_t *tree_dead;
    int32_t n_unfinished, finished;
};
int mld_debug_merge(mld_debug_merge_io *io)
{
    if (!io || !io->obj || !io->lbnd || !io->v || !io->status || !io->nodes || !io->pivots || !io->cuts || !io->refac || !io->rows || !io->item_root ||
        !io->item_label || !io->tree_dead) { mld_set_error("mld_debug_merge: null argument"); return MLD_ERR_INVALID; }
    const int batch = io->batch, cap = io->cap, n = io->n, tail = io->tail;
    if (batch < 1 || cap <= batch || tail < batch || tail > cap || n < 1 || (size_t)cap * (size_t)n > ((size_t)1 << 28)) {
        mld_set_error("mld_debug_merge: need 1 <= batch <= tail <= cap, cap > batch, n >= 1 (batch %d, tail %d, cap %d, n %d)", batch, tail, cap, n); return MLD_ERR_INVALID;
    }
    if (!(io->gap_abs >= 0.0) || !(io->gap_rel >= 0.0)) { mld_set_error("mld_debug_merge: gaps must be >= 0"); return MLD_ERR_INVALID; }
    for (int it = batch; it < tail; ++it) if (io->item_root[it] < 0 || io->item_root[it] >= batch) { mld_set_error("mld_debug_merge: item_root[%d] = %d is no root", it, io->item_root[it]); return MLD_ERR_INVALID; }
    for (int r = 0; r < batch; ++r) if (io->tree_dead[r] < 0 || io->tree_dead[r] > 2) { mld_set_error("mld_debug_merge: tree_dead[%d] = %d", r, io->tree_dead[r]); return MLD_ERR_INVALID; }
    const size_t c = cap, b = batch;
    DevBuf<double> obj, lbnd, v; DevBuf<int> status, nodes, pivots, cuts, refac, item_root, tree_dead, tl, unf, fin, mg_open;
    DevBuf<long long> rows, item_label; DevBuf<unsigned long long> mg_best, mg_lbopen, mg_label;
    HIP_TRY(obj.alloc(c)); HIP_TRY(lbnd.alloc(c)); HIP_TRY(v.alloc(c * n)); HIP_TRY(status.alloc(c)); HIP_TRY(nodes.alloc(c)); HIP_TRY(pivots.alloc(c));
    HIP_TRY(cuts.alloc(c)); HIP_TRY(refac.alloc(c)); HIP_TRY(rows.alloc(c)); HIP_TRY(item_root.alloc(c)); HIP_TRY(item_label.alloc(c)); HIP_TRY(tree_dead.alloc(b));
    HIP_TRY(tl.alloc(1)); HIP_TRY(unf.alloc(1)); HIP_TRY(fin.alloc(1));
    HIP_TRY(mg_best.alloc(b)); HIP_TRY(mg_lbopen.alloc(b)); HIP_TRY(mg_label.alloc(b)); HIP_TRY(mg_open.alloc(b));
    HIP_TRY(hipMemcpy(obj, io->obj, sizeof(double) * c, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(lbnd, io->lbnd, sizeof(double) * c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v, io->v, sizeof(double) * c * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(status, io->status, sizeof(int) * c, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(nodes, io->nodes, sizeof(int) * c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pivots, io->pivots, sizeof(int) * c, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(cuts, io->cuts, sizeof(int) * c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(refac, io->refac, sizeof(int) * c, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(rows, io->rows, sizeof(long long) * c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(item_root, io->item_root, sizeof(int) * c, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(item_label, io->item_label, sizeof(long long) * c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(tree_dead, io->tree_dead, sizeof(int) * b, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(tl, &tail, sizeof(int), hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(fin, &tail, sizeof(int), hipMemcpyHostToDevice));
    MergeArgs a;
    a.batch = batch; a.cap = cap; a.n = n; a.gap_abs = io->gap_abs; a.gap_rel = io->gap_rel;
    a.obj = obj; a.lbnd = lbnd; a.v = v; a.status = status; a.nodes = nodes; a.pivots = pivots; a.cuts = cuts; a.refac = refac; a.rows = rows;
    a.tail = tl; a.item_root = item_root; a.item_label = item_label; a.tree_dead = tree_dead;
    a.mg_best = mg_best; a.mg_lbopen = mg_lbopen; a.mg_label = mg_label; a.mg_open = mg_open; a.n_unfinished = unf; a.n_dead = fin;
    if (int rc = handoff_merge(a, 0)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(io->obj, obj, sizeof(double) * b, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(io->lbnd, lbnd, sizeof(double) * b, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(io->v, v, sizeof(double) * b * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(io->status, status, sizeof(int) * b, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(io->nodes, nodes, sizeof(int) * b, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(io->pivots, pivots, sizeof(int) * b, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(io->cuts, cuts, sizeof(int) * b, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(io->refac, refac, sizeof(int) * b, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(io->rows, rows, sizeof(long long) * b, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&io->n_unfinished, unf, sizeof(int), hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(&io->finished, fin, sizeof(int), hipMemcpyDeviceToHost));
    return MLD_OK;
}

int mld_advance_batch2(mld_problem_t *p, int32_t *n_skipped_out)
{
    MLD_NOT_IN_FLIGHT(p, "mld_advance_batch");
    if (!p || p->batch < 1) { mld_set_error("mld_advance_batch: nothing uploaded / solved"); return MLD_ERR_INVALID; }
    if (!p->solved) { mld_set_error("mld_advance_batch: the resident batch has not been solved since its upload / selection (there is no plan to apply)"); return MLD_ERR_INVALID; }
    if (p->advanced) { mld_set_error("mld_advance_batch: the last solve's plan has already been applied -- solve the advanced batch first (a second advance would apply the same step-0 inputs to a state that has moved on)"); return MLD_ERR_INVALID; }
    mld_model *m = p->model;
    const mld_dims &d = m->dims;
    if (!m->d_pack) { mld_set_error("mld_advance_batch: model without matrices"); return MLD_ERR_INVALID; }
    if (m->tv_N > 0) { mld_set_error("mld_advance_batch: time-varying models (mld_model_create_tv) are not advanced on the device -- the step models would have to shift with the horizon"); return MLD_ERR_INVALID; }
    /* offsets inside the packed per-model block: A, B4, b5, C, D4, d5, E, F4, f5, G, [B1 B2 B3 0], ...  (mld_model_create) */
    const size_t oA = 0, oB4 = oA + m->mat_size[MT_A], ob5 = oB4 + m->mat_size[MT_B4];
    size_t oBv = ob5 + m->mat_size[MT_b5];
    const int skip[7] = {MT_C, MT_D4, MT_d5, MT_E, MT_F4, MT_f5, MT_G};
    for (int k = 0; k < 7; ++k) oBv += m->mat_size[skip[k]];
    const size_t bx = ((size_t)p->batch * std::max(1, p->nx) + 255) / 256, bw = ((size_t)p->batch * std::max(1, p->nW) + 255) / 256;
    const int grid = (int)std::max<size_t>(bx, std::min<size_t>(bw, (size_t)1 << 20));   /* the state part is one thread per element, the shift strides */
    HIP_TRY(hipMemsetAsync(p->bat.skipped, 0, sizeof(int), p->stream));
    hipLaunchKernelGGL(k_advance, dim3(grid), dim3(256), 0, p->stream, p->batch, p->nx, p->nv, d.nomega, p->N,
                       m->d_pack, m->pack_len, 1, oA, oB4, ob5, oBv,
                       p->has_midx ? p->bat.model_idx : nullptr, p->bat.x0, p->bat.omega, p->bat.v, (size_t)p->n, p->bat.x0b, p->bat.omegab,
                       p->bat.status, p->bat.obj, p->bat.skipped);
    HIP_TRY(hipGetLastError());
    int skipped = 0;
    HIP_TRY(hipMemcpyAsync(&skipped, p->bat.skipped, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    std::swap(p->bat.x0, p->bat.x0b); std::swap(p->bat.omega, p->bat.omegab);
    p->n_xcols = 0;      /* extra constraint blocks belonged to the previous step's data */
    p->has_warm = false; /* a start belongs to one set of inputs (mld_warm_start_from_previous builds the next one from the plan) */
    p->has_cutoff = false;
    p->advanced = true;
    if (n_skipped_out) *n_skipped_out = skipped;
    return MLD_OK;
}

int mld_advance_batch(mld_problem_t *p) { return mld_advance_batch2(p, nullptr); }

int mld_set_warm_start(mld_problem_t *p, const uint8_t *bin_start)
{
    MLD_NOT_IN_FLIGHT(p, "mld_set_warm_start");
    if (!p || p->batch < 1) { mld_set_error("mld_set_warm_start: upload a batch first"); return MLD_ERR_INVALID; }
    if (!bin_start || p->nb == 0) { p->has_warm = false; return MLD_OK; }
    const size_t tot = (size_t)p->batch * p->nb;
    for (size_t k = 0; k < tot; ++k) if (bin_start[k] > 1 && bin_start[k] != 255) { mld_set_error("mld_set_warm_start: entry %zu is %d (0, 1, or 255 = no start)", k, (int)bin_start[k]); return MLD_ERR_INVALID; }
    HIP_TRY(hipMemcpy(p->bat.warm, bin_start, tot, hipMemcpyHostToDevice));
    p->has_warm = true;
    return MLD_OK;
}

int mld_warm_start_from_previous(mld_problem_t *p, int shift)
{
    MLD_NOT_IN_FLIGHT(p, "mld_warm_start_from_previous");
    if (!p || p->batch < 1 || shift < 0) { mld_set_error("mld_warm_start_from_previous: bad arguments"); return MLD_ERR_INVALID; }
    if (!p->solved) { mld_set_error("mld_warm_start_from_previous: the resident batch has no finished solve (its plan and statuses would be stale or uninitialised)"); return MLD_ERR_INVALID; }
    if (p->nb == 0) { p->has_warm = false; return MLD_OK; }
    const size_t tot = (size_t)p->batch * p->nb;
    hipLaunchKernelGGL(k_warm_from_plan, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, p->stream, p->batch, p->nb, p->nv, p->N, shift, p->d_bins,
                       p->bat.v, (size_t)p->n, p->bat.status, p->bat.obj, p->bat.warm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->has_warm = true;
    return MLD_OK;
}

int mld_set_cutoffs(mld_problem_t *p, const double *cutoff)
{
    MLD_NOT_IN_FLIGHT(p, "mld_set_cutoffs");
    if (!p || p->batch < 1) { mld_set_error("mld_set_cutoffs: upload a batch first"); return MLD_ERR_INVALID; }
    if (!cutoff) { p->has_cutoff = false; return MLD_OK; }
    HIP_TRY(hipMemcpy(p->bat.cutoff, cutoff, sizeof(double) * (size_t)p->batch, hipMemcpyHostToDevice));
    p->has_cutoff = true;
    return MLD_OK;
}

/* In-kernel sub-tree hand-off (DESIGN section 4d; the reference's one backend call per solve, controllers/controller_base.py:509, keeps every core of its
 * machine busy on ONE tree -- this is what lets one solve use more than one compute unit): an instance whose complete depth-first search stops at
 * max_nodes publishes its open nodes as queue entries of the SAME launch; idle workgroups solve them as instances of their own (sub_nodes each,
 * <= max_gen generations, a search with more than max_children open nodes is not split), and the results are merged into the instance on the device.
 * Takes effect with the next mld_upload_batch (the result arrays get room for room_factor x batch items, at least 4096). */
/* build(with_std_constraints=False) / set_constraints(std_evo_constaints=[...]) of the reference (controllers/mpc_controller.py:76-101,
 * controllers/controller_base.py:457-475): the standard block -- rows H_v v <= H_x x + H_w w + H_5 from the batch's own (x0, omega) -- is dropped, only
 * the blocks of mld_upload_constraint_blocks constrain; a row no block covers does not exist for that solve. */
int mld_set_std_block(mld_problem_t *p, int enable)
{
    MLD_NOT_IN_FLIGHT(p, "mld_set_std_block");
    if (!p) { mld_set_error("mld_set_std_block: bad handle"); return MLD_ERR_INVALID; }
    p->std_block = enable != 0;
    return MLD_OK;
}

int mld_set_handoff_policy(mld_problem_t *p, int donate, int rounds)
{
    MLD_NOT_IN_FLIGHT(p, "mld_set_handoff_policy");
    if (!p || donate < 0 || rounds < 0) { mld_set_error("mld_set_handoff_policy: bad arguments"); return MLD_ERR_INVALID; }
    p->ho_donate = std::min(donate, 64); p->ho_rounds = rounds;
    return MLD_OK;
}

int mld_set_handoff(mld_problem_t *p, int enable, int sub_nodes, int max_gen, int max_children, int max_tree, double room_factor)
{
    MLD_NOT_IN_FLIGHT(p, "mld_set_handoff");
    if (!p || sub_nodes < 0 || max_gen < 0 || max_children < 0) { mld_set_error("mld_set_handoff: bad arguments"); return MLD_ERR_INVALID; }
    if (enable && p->nb > 32000) { mld_set_error("mld_set_handoff: too many binaries"); return MLD_ERR_UNSUPPORTED; }
    const bool change = (enable != 0) != (p->ho_enable != 0) || (enable && room_factor > 0.0 && room_factor != p->ho_factor);
    p->ho_enable = enable ? 1 : 0;
    p->ho_sub_nodes = sub_nodes; p->ho_max_gen = max_gen > 0 ? max_gen : 8; p->ho_max_children = max_children > 0 ? max_children : 64;
    if (p->ho_max_gen > 8) p->ho_max_gen = 8;            /* (tree labels: 129^8 < 2^63) */
    if (p->ho_max_children > 64) p->ho_max_children = 64;
    p->ho_max_tree = max_tree > 0 ? max_tree : 160;
    if (room_factor > 0.0) p->ho_factor = room_factor;
    if (change) { free_batch(p); p->batch = 0; }         /* the result arrays are laid out anew by the next upload */
    return MLD_OK;
}

/* diagnostics (internal, not in the public header): per queue entry of the last hand-off solve -- in-kernel ticks, generation, status, root; returns the number of entries */
int mld_debug_entries(mld_problem_t *p, int cap, int64_t *ticks, int32_t *gen, int32_t *status, int32_t *root)
{
    if (!p || !p->ho_ran || !p->bat.ho.tail) return -1;
    int tl = 0;
    if (hipMemcpy(&tl, p->bat.ho.tail, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const int k = std::min(tl, cap);
    (void)hipMemcpy(ticks, p->bat.ticks, sizeof(long long) * k, hipMemcpyDeviceToHost);
    (void)hipMemcpy(status, p->bat.status, sizeof(int) * k, hipMemcpyDeviceToHost);
    if (k > p->batch) {
        (void)hipMemcpy(gen + p->batch, p->bat.ho.item_gen + p->batch, sizeof(int) * (k - p->batch), hipMemcpyDeviceToHost);
        (void)hipMemcpy(root + p->batch, p->bat.ho.item_root + p->batch, sizeof(int) * (k - p->batch), hipMemcpyDeviceToHost);
    }
    for (int i = 0; i < std::min(k, p->batch); ++i) { gen[i] = 0; root[i] = i; }
    return k;
}

/* out[0] items published by the last solve, out[1] reserved, out[2] instances left unfinished although they were split, out[3] entries the arrays have room for */
int mld_handoff_stats(mld_problem_t *p, int64_t out[4])
{
    if (!p || !out) { mld_set_error("mld_handoff_stats: bad arguments"); return MLD_ERR_INVALID; }
    for (int k = 0; k < 4; ++k) out[k] = p->ho_stats[k];
    return MLD_OK;
}

int mld_record_open_nodes(mld_problem_t *p, int enable)
{
    MLD_NOT_IN_FLIGHT(p, "mld_record_open_nodes");
    if (!p) { mld_set_error("mld_record_open_nodes: bad handle"); return MLD_ERR_INVALID; }
    if (enable && p->n > 32767) { mld_set_error("mld_record_open_nodes: the stacks store variable indices as int16 (n = %d > 32767)", p->n); return MLD_ERR_UNSUPPORTED; }
    p->want_open = enable != 0;
    return MLD_OK;
}

int mld_download_open_nodes(mld_problem_t *p, int32_t *depth_out, int16_t *var_out, uint8_t *val_out, uint8_t *flag_out)
{
    MLD_NOT_IN_FLIGHT(p, "mld_download_open_nodes");
    if (!p || p->batch < 1 || !p->solved || !p->want_open) { mld_set_error("mld_download_open_nodes: no finished solve with mld_record_open_nodes enabled"); return MLD_ERR_INVALID; }
    const size_t b = p->batch, nb = std::max(1, p->nb);
    if (depth_out) HIP_TRY(hipMemcpy(depth_out, p->bat.open_depth, sizeof(int) * b, hipMemcpyDeviceToHost));
    if (var_out) HIP_TRY(hipMemcpy(var_out, p->bat.open_var, sizeof(short) * b * nb, hipMemcpyDeviceToHost));
    if (val_out) HIP_TRY(hipMemcpy(val_out, p->bat.open_val, b * nb, hipMemcpyDeviceToHost));
    if (flag_out) HIP_TRY(hipMemcpy(flag_out, p->bat.open_flag, b * nb, hipMemcpyDeviceToHost));
    return MLD_OK;
}

int mld_stage_inputs(mld_problem_t *p, int n_sets, const double *x0_sets, const double *omega_sets)
{
    MLD_NOT_IN_FLIGHT(p, "mld_stage_inputs");
    if (!p || p->batch < 1) { mld_set_error("mld_stage_inputs: upload a batch first (it fixes the batch size and model_idx)"); return MLD_ERR_INVALID; }
    if (n_sets < 0 || (n_sets > 0 && ((p->nx && !x0_sets) || (p->nW && !omega_sets)))) { mld_set_error("mld_stage_inputs: bad arguments"); return MLD_ERR_INVALID; }
    p->bat.stage_x0.reset(); p->bat.stage_om.reset();
    p->n_staged = 0; p->staged_batch = 0;
    if (n_sets == 0) return MLD_OK;
    const size_t bx = (size_t)n_sets * p->batch * std::max(1, p->nx), bw = (size_t)n_sets * p->batch * std::max(1, p->nW);
    HIP_TRY(p->bat.stage_x0.alloc(bx));
    HIP_TRY(p->bat.stage_om.alloc(bw));
    if (p->nx) HIP_TRY(hipMemcpy(p->bat.stage_x0, x0_sets, sizeof(double) * (size_t)n_sets * p->batch * p->nx, hipMemcpyHostToDevice));
    if (p->nW) HIP_TRY(hipMemcpy(p->bat.stage_om, omega_sets, sizeof(double) * (size_t)n_sets * p->batch * p->nW, hipMemcpyHostToDevice));
    p->n_staged = n_sets; p->staged_batch = p->batch;
    return MLD_OK;
}

int mld_select_inputs(mld_problem_t *p, int set)
{
    MLD_NOT_IN_FLIGHT(p, "mld_select_inputs");
    if (!p || p->batch < 1 || p->staged_batch != p->batch || set < 0 || set >= p->n_staged) { mld_set_error("mld_select_inputs: set %d not staged for this batch", set); return MLD_ERR_INVALID; }
    if (p->nx) HIP_TRY(hipMemcpyAsync(p->bat.x0, p->bat.stage_x0 + (size_t)set * p->batch * p->nx, sizeof(double) * (size_t)p->batch * p->nx, hipMemcpyDeviceToDevice, p->stream));
    if (p->nW) HIP_TRY(hipMemcpyAsync(p->bat.omega, p->bat.stage_om + (size_t)set * p->batch * p->nW, sizeof(double) * (size_t)p->batch * p->nW, hipMemcpyDeviceToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));   /* the other entry points copy on the legacy stream, which does not order against a non-blocking one */
    p->n_xcols = 0;      /* extra constraint blocks belonged to the previous inputs */
    p->has_warm = false; p->solved = false; p->advanced = false; p->has_cutoff = false;
    return MLD_OK;
}

int mld_download_inputs(mld_problem_t *p, double *x0, double *omega)
{
    MLD_NOT_IN_FLIGHT(p, "mld_download_inputs");
    if (!p || p->batch < 1) { mld_set_error("mld_download_inputs: nothing uploaded"); return MLD_ERR_INVALID; }
    if (x0 && p->nx) HIP_TRY(hipMemcpy(x0, p->bat.x0, sizeof(double) * (size_t)p->batch * p->nx, hipMemcpyDeviceToHost));
    if (omega && p->nW) HIP_TRY(hipMemcpy(omega, p->bat.omega, sizeof(double) * (size_t)p->batch * p->nW, hipMemcpyDeviceToHost));
    return MLD_OK;
}

/* ---- resident disturbance profiles ----------------------------------------------------------------------------------------------------------------
 * The reference cuts every disturbance window out of a series it holds once (get_omega_tilde_k_hat / _act, modelling/micro_grid_agents.py:236-298;
 * get_omega_tilde_scenario, :206-232); here the series are a flat library in HBM and a window is a start offset (profiles.inc: k_profile_windows and the
 * window rule).  Every start is tested on the host before anything is queued: no kernel is launched with an offset that has not passed. */
int mld_upload_profiles(mld_problem_t *p, int64_t lib_len, const double *lib, int n_groups, const int32_t *group_width)
{
    if (mld_device_count() <= 0) { mld_set_error("no HIP device (libmldgpu has no CPU fallback)"); return MLD_ERR_NO_DEVICE; }
    MLD_NOT_IN_FLIGHT(p, "mld_upload_profiles");
    if (!p) { mld_set_error("mld_upload_profiles: null problem"); return MLD_ERR_INVALID; }
    const int nomega = p->model->dims.nomega;
    if (nomega == 0) { mld_set_error("mld_upload_profiles: the model has no disturbance (nomega = 0): there is nothing a profile could fill"); return MLD_ERR_INVALID; }
    if (lib_len < 0 || (lib_len > 0 && !lib)) { mld_set_error("mld_upload_profiles: lib_len = %lld%s", (long long)lib_len, lib_len > 0 ? " without a library" : ""); return MLD_ERR_INVALID; }
    if (n_groups < 0 || n_groups > nomega || (n_groups > 0 && !group_width)) { mld_set_error("mld_upload_profiles: n_groups = %d (0 .. nomega = %d, with group_width)", n_groups, nomega); return MLD_ERR_INVALID; }
    std::vector<int> width;
    if (n_groups == 0) width.assign(1, nomega);
    else {
        long long sum = 0;
        for (int g = 0; g < n_groups; ++g) {
            if (group_width[g] < 1) { mld_set_error("mld_upload_profiles: group_width[%d] = %d (every group needs at least one channel)", g, group_width[g]); return MLD_ERR_INVALID; }
            sum += group_width[g];
        }
        if (sum != nomega) { mld_set_error("mld_upload_profiles: the group widths sum to %lld, not to nomega = %d", sum, nomega); return MLD_ERR_INVALID; }
        width.assign(group_width, group_width + n_groups);
    }
    if (lib_len == 0) {      /* frees the library; the start arrays go with it */
        p->pf_lib.reset(); p->pf_chan.reset(); p->pf_fstart.reset(); p->pf_cstart.reset(); p->pf_astart.reset();
        p->pf_len = 0; p->pf_groups = 0; p->pf_width.clear(); p->pf_fbatch = p->pf_cbatch = p->pf_ccols = p->pf_abatch = 0;
        return MLD_OK;
    }
    std::vector<PfChan> chan;
    for (int g = 0; g < (int)width.size(); ++g) for (int o = 0; o < width[g]; ++o) chan.push_back(PfChan{g, o, width[g]});
    DevBuf<double> d_lib; DevBuf<PfChan> d_chan;      /* built beside the resident library: a call that fails leaves it as it was */
    HIP_TRY(d_lib.alloc((size_t)lib_len));
    HIP_TRY(d_chan.alloc(chan.size()));
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_lib, lib, sizeof(double) * (size_t)lib_len, hipMemcpyHostToDevice, sq));
        HIP_TRY(hipMemcpyAsync(d_chan, chan.data(), sizeof(PfChan) * chan.size(), hipMemcpyHostToDevice, sq));
        return MLD_OK;
    };
    const int rc = queue();
    const hipError_t es = hipStreamSynchronize(sq);
    if (rc) return rc;
    HIP_TRY(es);
    p->pf_lib = std::move(d_lib); p->pf_chan = std::move(d_chan);
    p->pf_len = lib_len; p->pf_groups = (int)width.size(); p->pf_width = width;
    p->pf_fstart.reset(); p->pf_cstart.reset(); p->pf_astart.reset(); p->pf_fbatch = p->pf_cbatch = p->pf_ccols = p->pf_abatch = 0;      /* starts pointed into the library that is gone */
    return MLD_OK;
}

/* what the three consumers share: a library and a step the window rule can be tested with */
static int profile_ready(const mld_problem *p, const char *who, int step)
{
    if (!p->pf_len) { mld_set_error("%s: no profile library resident (mld_upload_profiles)", who); return MLD_ERR_INVALID; }
    if (step < 0 || step > INT_MAX - p->N) { mld_set_error("%s: step = %d (must be >= 0)", who, step); return MLD_ERR_INVALID; }
    return MLD_OK;
}

/* every start of a (batch, n_cols, n_groups) array against the window rule; the first offender is named; gmax: per group the largest start */
static int profile_check_starts(const mld_problem *p, const char *who, const int64_t *start, int batch, int n_cols, int step, std::vector<long long> &gmax)
{
    const int G = p->pf_groups;
    gmax.assign(G, 0);
    const int64_t *s = start;
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < n_cols; ++c)
            for (int g = 0; g < G; ++g, ++s) {
                if (!profile_start_ok(*s, p->pf_len, step, p->N, p->pf_width[g])) {
                    mld_set_error("%s: start %lld of instance %d, column %d, group %d (width %d) at step %d: the window [%lld, %lld) leaves the library of %lld doubles",
                                  who, (long long)*s, b, c, g, p->pf_width[g], step, (long long)*s + (long long)step * p->pf_width[g],
                                  (long long)*s + ((long long)step + p->N) * p->pf_width[g], p->pf_len);
                    return MLD_ERR_INVALID;
                }
                gmax[g] = std::max<long long>(gmax[g], *s);
            }
    return MLD_OK;
}

/* resident starts under another step: the remembered maxima decide (the smallest start was >= 0 when the array was uploaded) */
static int profile_check_resident(const mld_problem *p, const char *who, const std::vector<long long> &gmax, int step)
{
    for (int g = 0; g < p->pf_groups; ++g)
        if (!profile_start_ok(gmax[g], p->pf_len, step, p->N, p->pf_width[g])) {
            mld_set_error("%s: step %d moves the largest resident start of group %d (%lld, width %d) past the end of the library: the window would end at %lld of %lld doubles",
                          who, step, g, gmax[g], p->pf_width[g], gmax[g] + ((long long)step + p->N) * p->pf_width[g], p->pf_len);
            return MLD_ERR_INVALID;
        }
    return MLD_OK;
}

static void launch_profile_windows(const mld_problem *p, hipStream_t sq, int rows, int cols, int ld_cols, int col0, const long long *d_start, int step, double *dst)
{
    const long long total = (long long)rows * p->nW;
    hipLaunchKernelGGL(k_profile_windows, dim3(profile_grid(total)), dim3(256), 0, sq, rows, p->nW, p->model->dims.nomega, cols, ld_cols, col0, p->pf_groups, d_start,
                       p->pf_chan.get(), step, p->pf_lib.get(), dst);
}

int mld_forecast_from_profiles(mld_problem_t *p, const int64_t *start, int step)
{
    static const char who[] = "mld_forecast_from_profiles";
    if (mld_device_count() <= 0) { mld_set_error("no HIP device (libmldgpu has no CPU fallback)"); return MLD_ERR_NO_DEVICE; }
    MLD_NOT_IN_FLIGHT(p, who);
    if (!p || p->batch < 1) { mld_set_error("%s: no batch resident (mld_upload_batch)", who); return MLD_ERR_INVALID; }
    int rc;
    if ((rc = profile_ready(p, who, step))) return rc;
    const int batch = p->batch, G = p->pf_groups;
    std::vector<long long> gmax;
    if (start) { if ((rc = profile_check_starts(p, who, start, batch, 1, step, gmax))) return rc; }
    else {
        if (p->pf_fbatch != batch) { mld_set_error("%s: start == NULL, but no starts of this batch are resident (pass them once)", who); return MLD_ERR_INVALID; }
        if ((rc = profile_check_resident(p, who, p->pf_fmax, step))) return rc;
    }
    DevBuf<long long> d_start;
    if (start) HIP_TRY(d_start.alloc((size_t)batch * G));
    const hipStream_t sq = p->stream;
    /* the new forecast is gathered into the spare input buffer and swapped in once the stream has finished: a call that fails changes nothing */
    auto queue = [&]() -> int {
        if (start) HIP_TRY(hipMemcpyAsync(d_start, start, sizeof(long long) * (size_t)batch * G, hipMemcpyHostToDevice, sq));
        launch_profile_windows(p, sq, batch, 1, 1, 0, start ? d_start.get() : p->pf_fstart.get(), step, p->bat.omegab.get());
        HIP_TRY(hipGetLastError());
        return MLD_OK;
    };
    rc = queue();
    const hipError_t es = hipStreamSynchronize(sq);
    if (rc) return rc;
    HIP_TRY(es);
    std::swap(p->bat.omega, p->bat.omegab);
    if (start) { p->pf_fstart = std::move(d_start); p->pf_fbatch = batch; p->pf_fmax = gmax; }
    if (!p->advanced) {      /* new inputs, as mld_select_inputs; after mld_advance_batch the blocks are gone already and plan and start stay */
        p->n_xcols = 0;
        p->has_warm = false; p->solved = false; p->has_cutoff = false;
    }
    return MLD_OK;
}

int mld_constraint_blocks_from_profiles(mld_problem_t *p, int n_cols, const int64_t *start, int step, const int32_t *col_rows, const double *x_cols)
{
    static const char who[] = "mld_constraint_blocks_from_profiles";
    if (mld_device_count() <= 0) { mld_set_error("no HIP device (libmldgpu has no CPU fallback)"); return MLD_ERR_NO_DEVICE; }
    MLD_NOT_IN_FLIGHT(p, who);
    if (!p || p->batch < 1) { mld_set_error("%s: upload the batch first", who); return MLD_ERR_INVALID; }
    if (n_cols < 0) { mld_set_error("%s: n_cols = %d", who, n_cols); return MLD_ERR_INVALID; }
    if (n_cols == 0) { p->n_xcols = 0; return MLD_OK; }
    int rc;
    if ((rc = profile_ready(p, who, step))) return rc;
    const int batch = p->batch, G = p->pf_groups;
    if ((long long)batch * n_cols > INT_MAX) { mld_set_error("%s: batch x n_cols = %lld windows (at most %d)", who, (long long)batch * n_cols, INT_MAX); return MLD_ERR_INVALID; }
    if (col_rows) for (int c = 0; c < n_cols; ++c) if (col_rows[c] < 0 || col_rows[c] > p->m0) { mld_set_error("%s: col_rows[%d]=%d outside [0,%d]", who, c, col_rows[c], p->m0); return MLD_ERR_INVALID; }
    std::vector<long long> gmax;
    if (start) { if ((rc = profile_check_starts(p, who, start, batch, n_cols, step, gmax))) return rc; }
    else {
        if (p->pf_cbatch != batch) { mld_set_error("%s: start == NULL, but no column starts of this batch are resident (pass them once)", who); return MLD_ERR_INVALID; }
        if (p->pf_ccols != n_cols) { mld_set_error("%s: start == NULL with n_cols = %d, but the resident starts are those of %d columns", who, n_cols, p->pf_ccols); return MLD_ERR_INVALID; }
        if ((rc = profile_check_resident(p, who, p->pf_cmax, step))) return rc;
    }
    /* from here on as mld_upload_constraint_blocks_x, with the gather in place of the copy of omega_cols */
    DevBuf<long long> d_start;
    if (start) HIP_TRY(d_start.alloc((size_t)batch * n_cols * G));
    p->n_xcols = 0;
    const size_t need = (size_t)batch * n_cols * p->nW;
    if (need > p->xcols_cap) {
        p->xcols_cap = 0;
        HIP_TRY(p->bat.xcols.alloc(need));
        p->xcols_cap = need;
    }
    p->bat.xrows.reset();
    if (col_rows) HIP_TRY(p->bat.xrows.alloc(n_cols));
    p->has_xcols_x = false;
    const bool with_x = x_cols && p->nx;
    const size_t nxs = (size_t)batch * n_cols * p->nx;
    if (with_x) HIP_TRY(p->bat.xcols_x.alloc(nxs));
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int {
        if (start) HIP_TRY(hipMemcpyAsync(d_start, start, sizeof(long long) * (size_t)batch * n_cols * G, hipMemcpyHostToDevice, sq));
        if (col_rows) HIP_TRY(hipMemcpyAsync(p->bat.xrows, col_rows, sizeof(int) * n_cols, hipMemcpyHostToDevice, sq));
        if (with_x) HIP_TRY(hipMemcpyAsync(p->bat.xcols_x, x_cols, sizeof(double) * nxs, hipMemcpyHostToDevice, sq));
        launch_profile_windows(p, sq, batch * n_cols, n_cols, n_cols, 0, start ? d_start.get() : p->pf_cstart.get(), step, p->bat.xcols.get());
        HIP_TRY(hipGetLastError());
        return MLD_OK;
    };
    rc = queue();
    const hipError_t es = hipStreamSynchronize(sq);
    if (rc) return rc;
    HIP_TRY(es);
    if (start) { p->pf_cstart = std::move(d_start); p->pf_cbatch = batch; p->pf_ccols = n_cols; p->pf_cmax = gmax; }
    p->has_xcols_x = with_x;
    p->n_xcols = n_cols;
    return MLD_OK;
}

int mld_download_constraint_blocks(mld_problem_t *p, int32_t *n_cols_out, double *omega_cols, int32_t *col_rows, double *x_cols)
{
    MLD_NOT_IN_FLIGHT(p, "mld_download_constraint_blocks");
    if (!p || p->batch < 1) { mld_set_error("mld_download_constraint_blocks: nothing uploaded"); return MLD_ERR_INVALID; }
    const int nc = p->n_xcols;
    if (x_cols && nc && !p->has_xcols_x) { mld_set_error("mld_download_constraint_blocks: x_cols asked for, but the resident blocks have none (every column uses the instance's x0)"); return MLD_ERR_INVALID; }
    if (n_cols_out) *n_cols_out = nc;
    if (!nc) return MLD_OK;
    if (omega_cols) HIP_TRY(hipMemcpy(omega_cols, p->bat.xcols, sizeof(double) * (size_t)p->batch * nc * p->nW, hipMemcpyDeviceToHost));
    if (col_rows) {
        if (p->bat.xrows) HIP_TRY(hipMemcpy(col_rows, p->bat.xrows, sizeof(int) * nc, hipMemcpyDeviceToHost));
        else for (int c = 0; c < nc; ++c) col_rows[c] = p->m0;
    }
    if (x_cols) HIP_TRY(hipMemcpy(x_cols, p->bat.xcols_x, sizeof(double) * (size_t)p->batch * nc * p->nx, hipMemcpyDeviceToHost));
    return MLD_OK;
}

/* Per-instance linear cost of the resident batch (the reference rebuilds its objective with the current tariff before every solve() call,
 * micro_grid_control_simulation.py:194-198,229: N calls replaced by one batch may carry N price vectors).  Weights on v are kept as uploaded; weights on
 * x_tilde / y_tilde are pulled back through the tightened model's condensed maps by ONE GEMM per model (k_inst_pullback; k_inst_pullback_valu under
 * MLD_DBG_GEMM_VALU) into [q_b | cx_b | cw_b | c0_b].  The new cost is built in a buffer of its own: a call that fails leaves the resident one as it was. */
int mld_upload_instance_cost(mld_problem_t *p, const double *lin_v, const double *lin_x, const double *lin_y)
{
    if (mld_device_count() <= 0) { mld_set_error("no HIP device (libmldgpu has no CPU fallback)"); return MLD_ERR_NO_DEVICE; }
    MLD_NOT_IN_FLIGHT(p, "mld_upload_instance_cost");
    if (!p || p->batch < 1) { mld_set_error("mld_upload_instance_cost: upload a batch first (the cost belongs to its instances)"); return MLD_ERR_INVALID; }
    const int n = p->n, nx = p->nx, nW = p->nW, batch = p->batch;
    const int NX = p->N * p->model->dims.nx, NY = p->N * p->model->dims.ny;
    if (lin_x && NX == 0) { mld_set_error("mld_upload_instance_cost: lin_x given but the model has no state (nx = 0)"); return MLD_ERR_INVALID; }
    if (lin_y && NY == 0) { mld_set_error("mld_upload_instance_cost: lin_y given but the model has no output (ny = 0)"); return MLD_ERR_INVALID; }
    if (!lin_v && !lin_x && !lin_y) { p->bat.icost.reset(); p->bat.qs_inst_t.reset(); p->ic_ld = 0; return MLD_OK; }
    const hipStream_t sq = p->stream;
    const bool pull = lin_x || lin_y;
    const int ld = pull ? n + nx + nW + 1 : n;      /* weights on v only: no GEMM, cx / cw / c0 are zero and not stored */
    DevBuf<double> ic, d_w;
    HIP_TRY(ic.alloc((size_t)batch * std::max(1, ld)));
    /* everything queued on the stream; the wait below comes on EVERY path, so that the caller's arrays and the temporaries may go when this returns */
    auto queue = [&]() -> int {
    if (!lin_v || pull) HIP_TRY(hipMemsetAsync(ic, 0, sizeof(double) * (size_t)batch * std::max(1, ld), sq));
    if (lin_v && n && !pull) HIP_TRY(hipMemcpyAsync(ic, lin_v, sizeof(double) * (size_t)batch * n, hipMemcpyHostToDevice, sq));      /* rows are contiguous: one plain copy */
    else if (lin_v && n) HIP_TRY(hipMemcpy2DAsync(ic, sizeof(double) * ld, lin_v, sizeof(double) * n, sizeof(double) * n, batch, hipMemcpyHostToDevice, sq));
    if (pull) {
        const int K = NX + NY;
        const mld_model *t = p->tight.get();
        HIP_TRY(d_w.alloc((size_t)batch * K));
        if (!lin_x || !lin_y) HIP_TRY(hipMemsetAsync(d_w, 0, sizeof(double) * (size_t)batch * K, sq));
        if (lin_x) HIP_TRY(hipMemcpy2DAsync(d_w, sizeof(double) * K, lin_x, sizeof(double) * NX, sizeof(double) * NX, batch, hipMemcpyHostToDevice, sq));
        if (lin_y) HIP_TRY(hipMemcpy2DAsync(d_w.get() + NX, sizeof(double) * K, lin_y, sizeof(double) * NY, sizeof(double) * NY, batch, hipMemcpyHostToDevice, sq));
        PbMaps mp;
        const int oW[4] = {O_GamV, O_PhiX, O_GamW, O_Gam5}, oY[4] = {O_LV, O_LX, O_LW, O_L5};
        for (int f = 0; f < 4; ++f) {
            mp.W[f] = NX ? t->d_out[oW[f]].get() : nullptr; mp.sW[f] = t->lay.out_size[oW[f]];
            mp.Y[f] = NY ? t->d_out[oY[f]].get() : nullptr; mp.sY[f] = t->lay.out_size[oY[f]];
        }
        if (p->opts.reserved & MLD_DBG_GEMM_VALU)
            hipLaunchKernelGGL(k_inst_pullback_valu, dim3(batch), dim3(256), sizeof(double) * K, sq, NX, NY, n, nx, nW, mp, p->has_midx ? p->bat.model_idx.get() : nullptr, d_w.get(), ic.get());
        else if (p->opts.flags & MLD_F32)
            hipLaunchKernelGGL(k_inst_pullback<true>, dim3(p->n_groups), dim3(64 * RM_WAVES), 0, sq, NX, NY, n, nx, nW, mp, p->bat.groups.get(), p->bat.perm.get(), d_w.get(), ic.get());
        else
            hipLaunchKernelGGL(k_inst_pullback<false>, dim3(p->n_groups), dim3(64 * RM_WAVES), 0, sq, NX, NY, n, nx, nW, mp, p->bat.groups.get(), p->bat.perm.get(), d_w.get(), ic.get());
        HIP_TRY(hipGetLastError());
    }
    return MLD_OK;
    };
    const int rc = queue();
    const hipError_t es = hipStreamSynchronize(sq);
    if (rc) return rc;
    HIP_TRY(es);
    p->bat.icost = std::move(ic); p->ic_ld = ld;
    return MLD_OK;
}

int mld_download_instance_cost(mld_problem_t *p, double *q_out, double *const_out)
{
    MLD_NOT_IN_FLIGHT(p, "mld_download_instance_cost");
    if (!p || p->batch < 1) { mld_set_error("mld_download_instance_cost: nothing uploaded"); return MLD_ERR_INVALID; }
    const size_t b = p->batch, n = p->n;
    if (!p->ic_ld) {
        if (q_out) memset(q_out, 0, sizeof(double) * b * n);
        if (const_out) memset(const_out, 0, sizeof(double) * b);
        return MLD_OK;
    }
    if (q_out && n) HIP_TRY(hipMemcpy2D(q_out, sizeof(double) * n, p->bat.icost, sizeof(double) * p->ic_ld, sizeof(double) * n, b, hipMemcpyDeviceToHost));
    if (const_out) {
        memset(const_out, 0, sizeof(double) * b);
        if (p->ic_ld > p->n) {
            DevBuf<double> d_c;
            HIP_TRY(d_c.alloc(b));
            HIP_TRY(hipMemsetAsync(d_c, 0, sizeof(double) * b, p->stream));
            hipLaunchKernelGGL(k_inst_const, dim3((p->batch + 3) / 4), dim3(256), 0, p->stream, p->batch, p->n, p->nx, p->nW, p->ic_ld, p->bat.icost, p->bat.x0, p->bat.omega, d_c.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(const_out, d_c, sizeof(double) * b, hipMemcpyDeviceToHost, p->stream));
            HIP_TRY(hipStreamSynchronize(p->stream));
        }
    }
    return MLD_OK;
}

/* Predicted state and output trajectories of the resident batch (gen_state_output_vars, controllers/components/variables.py:246-286: x_tilde :259-265,
 * y_tilde :269-275, with its variables= / x_k= / omega_tilde_k= arguments) as ONE GEMM per model over [v | x0 | omega | 1] (k_trajectory;
 * k_trajectory_valu under MLD_DBG_GEMM_VALU).  The state and output maps of the tightened model are the original ones (tightening changes F1 / F2 / Psi
 * and f5 only).  v == NULL: the resident solution, rows of instances without a usable plan all NaN; v given: the caller's plans under the current inputs.
 * The results are built in buffers of their own and every path waits for the stream, so a call that fails changes nothing. */
int mld_predict_batch(mld_problem_t *p, const double *v, double *x_out, double *y_out)
{
    if (mld_device_count() <= 0) { mld_set_error("no HIP device (libmldgpu has no CPU fallback)"); return MLD_ERR_NO_DEVICE; }
    MLD_NOT_IN_FLIGHT(p, "mld_predict_batch");
    if (!p || p->batch < 1) { mld_set_error("mld_predict_batch: no batch resident (mld_upload_batch)"); return MLD_ERR_INVALID; }
    const mld_dims &d = p->model->dims;
    const int n = p->n, nx = p->nx, nW = p->nW, batch = p->batch, N = p->N;
    const int NX = N * d.nx, NY = N * d.ny;
    if (x_out && NX == 0) { mld_set_error("mld_predict_batch: x_out given but the model has no state (nx = 0)"); return MLD_ERR_INVALID; }
    if (y_out && NY == 0) { mld_set_error("mld_predict_batch: y_out given but the model has no output (ny = 0)"); return MLD_ERR_INVALID; }
    if (!v && !p->solved) { mld_set_error("mld_predict_batch: the resident batch has not been solved since its upload / selection (there is no plan to evaluate; pass v)"); return MLD_ERR_INVALID; }
    if (!v && p->advanced) { mld_set_error("mld_predict_batch: mld_advance_batch has moved the inputs on -- the resident plan belongs to inputs that are gone (solve again, or pass v)"); return MLD_ERR_INVALID; }
    if (!x_out && !y_out) return MLD_OK;
    const hipStream_t sq = p->stream;
    DevBuf<double> d_v, d_x, d_y;
    if (x_out) HIP_TRY(d_x.alloc((size_t)batch * NX));
    if (y_out) HIP_TRY(d_y.alloc((size_t)batch * NY));
    if (v) HIP_TRY(d_v.alloc((size_t)batch * std::max(1, n)));
    /* everything queued on the stream; the wait below comes on EVERY path, so that the caller's arrays and the temporaries may go when this returns */
    auto queue = [&]() -> int {
        if (v && n) HIP_TRY(hipMemcpyAsync(d_v, v, sizeof(double) * (size_t)batch * n, hipMemcpyHostToDevice, sq));
        const double *pv = v ? d_v.get() : p->bat.v.get();      /* (the resident solution: rows < batch are the instances', hand-off items come after them) */
        const int *st = v ? nullptr : p->bat.status.get();
        const double *ob = v ? nullptr : p->bat.obj.get();
        const mld_model *t = p->tight.get();
        PbMaps mp;
        const int oW[4] = {O_GamV, O_PhiX, O_GamW, O_Gam5}, oY[4] = {O_LV, O_LX, O_LW, O_L5};
        for (int f = 0; f < 4; ++f) {
            mp.W[f] = NX ? t->d_out[oW[f]].get() : nullptr; mp.sW[f] = t->lay.out_size[oW[f]];
            mp.Y[f] = NY ? t->d_out[oY[f]].get() : nullptr; mp.sY[f] = t->lay.out_size[oY[f]];
        }
        const int r_begin = x_out ? 0 : NX, r_end = y_out ? NX + NY : NX;      /* rows of the stacked maps that are asked for */
        if (p->opts.reserved & MLD_DBG_GEMM_VALU)
            hipLaunchKernelGGL(k_trajectory_valu, dim3(batch), dim3(256), sizeof(double) * (n + nx + nW + 1), sq, NX, NY, n, nx, nW, mp,
                               p->has_midx ? p->bat.model_idx.get() : nullptr, pv, p->bat.x0.get(), p->bat.omega.get(), st, ob, r_begin, r_end, d_x.get(), d_y.get());
        else if (p->opts.flags & MLD_F32)
            hipLaunchKernelGGL(k_trajectory<true>, dim3(p->n_groups), dim3(64 * RM_WAVES), 0, sq, N, d.nx, d.ny, p->nv, d.nomega, mp, p->bat.groups.get(), p->bat.perm.get(),
                               pv, p->bat.x0.get(), p->bat.omega.get(), st, ob, r_begin, r_end, d_x.get(), d_y.get());
        else
            hipLaunchKernelGGL(k_trajectory<false>, dim3(p->n_groups), dim3(64 * RM_WAVES), 0, sq, N, d.nx, d.ny, p->nv, d.nomega, mp, p->bat.groups.get(), p->bat.perm.get(),
                               pv, p->bat.x0.get(), p->bat.omega.get(), st, ob, r_begin, r_end, d_x.get(), d_y.get());
        HIP_TRY(hipGetLastError());
        if (x_out) HIP_TRY(hipMemcpyAsync(x_out, d_x, sizeof(double) * (size_t)batch * NX, hipMemcpyDeviceToHost, sq));
        if (y_out) HIP_TRY(hipMemcpyAsync(y_out, d_y, sizeof(double) * (size_t)batch * NY, hipMemcpyDeviceToHost, sq));
        return MLD_OK;
    };
    const int rc = queue();
    const hipError_t es = hipStreamSynchronize(sq);
    if (rc) return rc;
    HIP_TRY(es);
    return MLD_OK;
}

/* Solution quality of the resident batch: what the reference's backend reports after every solve (ObjVal, ConstrVio, IntVio, BoundVio;
 * controllers/controller_base.py:509) for the resident or the caller's plans, on the ORIGINAL model's rows (condensed on first use, as mld_rhs_batch
 * does) and any disturbance columns (the layout of gen_evo_constraints, controller_base.py:411-456).  Kernels: evaluate.inc.  Every result is built
 * in a buffer of its own and every path waits for the stream, so a call that fails changes nothing; nothing the solve path reads is written. */
#define EV_SLICE_BYTES ((size_t)256 << 20)      /* device copy of the caller's validation columns: at most this much at a time (at least one column) */
/* The columns of a call come from one of two sources: the caller's array (omega_cols, mld_evaluate_batch) or starts into the resident profile library
 * (start / step, mld_evaluate_batch_profiles: from_profiles).  The sources differ in how a slice of columns reaches the slice buffer d_om -- a strided copy
 * from the host, or k_profile_windows gathering it there -- and in nothing else: the same slices, the same launches of k_evaluate on the same buffer. */
static int evaluate_impl(mld_problem_t *p, const char *who, const double *v, int n_cols, const double *omega_cols, bool from_profiles, const int64_t *start, int step,
                         const int32_t *col_rows, const double *x_cols,
                         double *obj_out, double *constr_vio_out, int32_t *constr_row_out, double *int_vio_out, double *bound_vio_out)
{
    if (mld_device_count() <= 0) { mld_set_error("no HIP device (libmldgpu has no CPU fallback)"); return MLD_ERR_NO_DEVICE; }
    MLD_NOT_IN_FLIGHT(p, who);
    if (!p || p->batch < 1) { mld_set_error("%s: no batch resident (mld_upload_batch)", who); return MLD_ERR_INVALID; }
    const mld_dims &d = p->model->dims;
    const int n = p->n, nx = p->nx, nW = p->nW, batch = p->batch, m0 = p->m0, M = p->n_models;
    if (n_cols < 0) { mld_set_error("%s: n_cols = %d", who, n_cols); return MLD_ERR_INVALID; }
    if (!from_profiles && n_cols > 0 && nW && !omega_cols) { mld_set_error("%s: n_cols = %d without omega_cols (nomega > 0)", who, n_cols); return MLD_ERR_INVALID; }
    if (from_profiles && n_cols < 1) { mld_set_error("%s: n_cols = %d (the profile columns of a call: at least one)", who, n_cols); return MLD_ERR_INVALID; }
    if (from_profiles && !start) { mld_set_error("%s: start == NULL (the resident column starts belong to the problem's blocks and are not used here)", who); return MLD_ERR_INVALID; }
    if (x_cols && nx == 0) { mld_set_error("%s: x_cols given but the model has no state (nx = 0)", who); return MLD_ERR_INVALID; }
    if (col_rows) for (int c = 0; c < n_cols; ++c) if (col_rows[c] < 0 || col_rows[c] > m0) { mld_set_error("%s: col_rows[%d]=%d outside [0,%d]", who, c, col_rows[c], m0); return MLD_ERR_INVALID; }
    if (!v && !p->solved) { mld_set_error("%s: the resident batch has not been solved since its upload / selection (there is no plan to evaluate; pass v)", who); return MLD_ERR_INVALID; }
    if (!v && p->advanced) { mld_set_error("%s: mld_advance_batch has moved the inputs on -- the resident plan belongs to inputs that are gone (solve again, or pass v)", who); return MLD_ERR_INVALID; }
    int rc;
    if (from_profiles) {      /* every start against the window rule, before anything is queued */
        std::vector<long long> gmax;
        if ((rc = profile_ready(p, who, step))) return rc;
        if ((long long)batch * n_cols > INT_MAX) { mld_set_error("%s: batch x n_cols = %lld windows (at most %d)", who, (long long)batch * n_cols, INT_MAX); return MLD_ERR_INVALID; }
        if ((rc = profile_check_starts(p, who, start, batch, n_cols, step, gmax))) return rc;
    }
    if (!obj_out && !constr_vio_out && !constr_row_out && !int_vio_out && !bound_vio_out) return MLD_OK;
    const hipStream_t sq = p->stream;
    const bool want_c = constr_vio_out || constr_row_out;
    const bool valu = (p->opts.reserved & MLD_DBG_GEMM_VALU) != 0;
    mld_model *mo = p->model;
    if (want_c && m0 && (mo->cond_N != p->N || !mo->out64) && (rc = condense_model_device(mo, p->N, nullptr, sq))) return rc;
    const int *midx = p->has_midx ? p->bat.model_idx.get() : nullptr;
    const size_t nout = n_cols > 0 ? (size_t)n_cols : 1;      /* constraint results per instance */
    /* columns of the caller per launch: the device copy of a slice stays within EV_SLICE_BYTES */
    const size_t col_bytes = sizeof(double) * (size_t)batch * std::max(1, nW + (x_cols ? nx : 0));
    const int slice = n_cols > 0 ? (int)std::min<size_t>((size_t)n_cols, std::max<size_t>(1, EV_SLICE_BYTES / col_bytes)) : 0;
    DevBuf<double> d_v, d_hv, d_part, d_om, d_xc, d_vio, d_obj, d_iv, d_bv, d_qi, d_rc, d_one;
    DevBuf<int> d_rows, d_row; DevBuf<long long> d_start;
    if (v) HIP_TRY(d_v.alloc((size_t)batch * std::max(1, n)));
    if (want_c) {
        HIP_TRY(d_hv.alloc((size_t)batch * std::max(1, m0)));
        if (!valu && nx + nW > EV_KC) HIP_TRY(d_part.alloc((size_t)batch * std::max(1, m0)));
        HIP_TRY(d_vio.alloc((size_t)batch * nout)); HIP_TRY(d_row.alloc((size_t)batch * nout));
        if (slice && nW) HIP_TRY(d_om.alloc((size_t)batch * slice * nW));
        if (slice && x_cols) HIP_TRY(d_xc.alloc((size_t)batch * slice * nx));
        if (slice && col_rows) HIP_TRY(d_rows.alloc(n_cols));
        if (from_profiles) HIP_TRY(d_start.alloc((size_t)batch * n_cols * p->pf_groups));
    }
    const bool inst_q = p->has_quad || p->ic_ld;
    if (obj_out) {
        HIP_TRY(d_obj.alloc(batch));
        if (inst_q) { HIP_TRY(d_qi.alloc((size_t)batch * std::max(1, n))); HIP_TRY(d_rc.alloc(batch)); HIP_TRY(d_one.alloc((size_t)std::max(1, n) * M)); }
    }
    if (int_vio_out) HIP_TRY(d_iv.alloc(batch));
    if (bound_vio_out) HIP_TRY(d_bv.alloc(batch));
    /* everything queued on the stream; the wait below comes on EVERY path, so that the caller's arrays and the temporaries may go when this returns */
    auto queue = [&]() -> int {
        if (v && n) HIP_TRY(hipMemcpyAsync(d_v, v, sizeof(double) * (size_t)batch * n, hipMemcpyHostToDevice, sq));
        const double *pv = v ? d_v.get() : p->bat.v.get();      /* (the resident solution: rows < batch are the instances', after the hand-off's merge) */
        const int *st = v ? nullptr : p->bat.status.get();
        const double *ob = v ? nullptr : p->bat.obj.get();
        if (want_c) {
            EvCols ec;
            ec.x0 = p->bat.x0.get(); ec.omega = p->bat.omega.get();
            const double *Hv = m0 ? mo->d_out[O_HV].get() : nullptr, *Hx = m0 && nx ? mo->d_out[O_HX].get() : nullptr;
            const double *Hw = m0 && nW ? mo->d_out[O_HW].get() : nullptr, *H5 = m0 ? mo->d_out[O_H5].get() : nullptr;
            auto launch_ev = [&](int do_v) {
                if (valu)
                    hipLaunchKernelGGL(k_evaluate_valu, dim3(batch), dim3(256), sizeof(double) * (n + m0), sq, m0, n, nx, nW, Hv, Hx, Hw, H5, midx, pv, st, ob, do_v, ec,
                                       d_hv.get(), d_vio.get(), d_row.get());
                else
                    hipLaunchKernelGGL(k_evaluate, dim3(p->n_groups), dim3(64 * RM_WAVES), 0, sq, m0, std::max(1, d.nc), p->nv, d.nomega, n, nx, nW, Hv, Hx, Hw, H5,
                                       p->bat.groups.get(), p->bat.perm.get(), pv, st, ob, do_v, ec, d_hv.get(), d_part.get(), d_vio.get(), d_row.get());
            };
            if (n_cols == 0) {      /* the problem as posed: the columns the next solve would enforce */
                ec.n_cols = p->n_xcols; ec.std = p->std_block ? 1 : 0; ec.per_col = 0; ec.ld_out = 1; ec.col0 = 0;
                ec.omc = p->bat.xcols.get(); ec.xc = p->has_xcols_x ? p->bat.xcols_x.get() : nullptr; ec.rows = p->n_xcols ? p->bat.xrows.get() : nullptr;
                launch_ev(1);
            } else {
                if (col_rows) HIP_TRY(hipMemcpyAsync(d_rows, col_rows, sizeof(int) * n_cols, hipMemcpyHostToDevice, sq));
                if (from_profiles) HIP_TRY(hipMemcpyAsync(d_start, start, sizeof(long long) * (size_t)batch * n_cols * p->pf_groups, hipMemcpyHostToDevice, sq));
                for (int c0 = 0; c0 < n_cols; c0 += slice) {
                    const int nc_ = std::min(slice, n_cols - c0);
                    if (from_profiles) { launch_profile_windows(p, sq, batch * nc_, nc_, n_cols, c0, d_start.get(), step, d_om.get()); HIP_TRY(hipGetLastError()); }
                    else if (nW) HIP_TRY(hipMemcpy2DAsync(d_om, sizeof(double) * nc_ * nW, omega_cols + (size_t)c0 * nW, sizeof(double) * n_cols * nW, sizeof(double) * nc_ * nW, batch, hipMemcpyHostToDevice, sq));
                    if (x_cols) HIP_TRY(hipMemcpy2DAsync(d_xc, sizeof(double) * nc_ * nx, x_cols + (size_t)c0 * nx, sizeof(double) * n_cols * nx, sizeof(double) * nc_ * nx, batch, hipMemcpyHostToDevice, sq));
                    ec.n_cols = nc_; ec.std = 0; ec.per_col = 1; ec.ld_out = n_cols; ec.col0 = c0;
                    ec.omc = d_om.get(); ec.xc = x_cols ? d_xc.get() : nullptr; ec.rows = col_rows ? d_rows.get() + c0 : nullptr;
                    launch_ev(c0 == 0);
                    HIP_TRY(hipGetLastError());
                }
            }
            HIP_TRY(hipGetLastError());
            if (constr_vio_out) HIP_TRY(hipMemcpyAsync(constr_vio_out, d_vio, sizeof(double) * (size_t)batch * nout, hipMemcpyDeviceToHost, sq));
            if (constr_row_out) HIP_TRY(hipMemcpyAsync(constr_row_out, d_row, sizeof(int) * (size_t)batch * nout, hipMemcpyDeviceToHost, sq));
        }
        if (int_vio_out || bound_vio_out) {
            hipLaunchKernelGGL(k_eval_point, dim3((batch + 3) / 4), dim3(256), 0, sq, batch, n, p->nv, d.nu, d.nu_l, d.ndelta, d.nz, d.nmu, d.nmu_l, pv, st, ob, d_iv.get(), d_bv.get());
            HIP_TRY(hipGetLastError());
            if (int_vio_out) HIP_TRY(hipMemcpyAsync(int_vio_out, d_iv, sizeof(double) * batch, hipMemcpyDeviceToHost, sq));
            if (bound_vio_out) HIP_TRY(hipMemcpyAsync(bound_vio_out, d_bv, sizeof(double) * batch, hipMemcpyDeviceToHost, sq));
        }
        if (obj_out) {
            /* the per-instance q and constant at the current inputs by the kernels of launch_rhs_cost / launch_inst_cost, with unit column scales and
             * into buffers of this call (the solve path's qs_inst / rconst are not touched) */
            if (inst_q) {
                const size_t tot = (size_t)batch * n, one = (size_t)std::max(1, n) * M;
                hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)((one + 255) / 256)), dim3(256), 0, sq, one, 1.0, d_one.get());
                HIP_TRY(hipMemsetAsync(d_rc, 0, sizeof(double) * batch, sq));
                if (p->has_quad) {
                    const mld_model *t = p->tight.get();
                    const int NX = p->N * d.nx, NY = p->N * d.ny;
                    hipLaunchKernelGGL(k_qinst, dim3(batch), dim3(256), 0, sq, n, nx, nW, p->d_q0, p->d_Qx, p->d_Qw, d_one.get(), midx, p->bat.x0, p->bat.omega, d_qi.get(),
                                       p->ic_ld ? p->bat.icost.get() : nullptr, p->ic_ld);
                    if (p->d_Wx && NX) hipLaunchKernelGGL(k_quad_const, dim3(batch), dim3(256), sizeof(double) * NX, sq, NX, nx, nW, t->d_out[O_PhiX], t->lay.out_size[O_PhiX],
                                                          t->d_out[O_GamW], t->lay.out_size[O_GamW], t->d_out[O_Gam5], t->lay.out_size[O_Gam5], p->d_Wx, midx, p->bat.x0, p->bat.omega, d_rc.get());
                    if (p->d_Wy && NY) hipLaunchKernelGGL(k_quad_const, dim3(batch), dim3(256), sizeof(double) * NY, sq, NY, nx, nW, t->d_out[O_LX], t->lay.out_size[O_LX],
                                                          t->d_out[O_LW], t->lay.out_size[O_LW], t->d_out[O_L5], t->lay.out_size[O_L5], p->d_Wy, midx, p->bat.x0, p->bat.omega, d_rc.get());
                } else if (tot)
                    hipLaunchKernelGGL(k_inst_cost, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, sq, tot, n, p->ic_ld, p->d_q0, d_one.get(), (const double *)nullptr, midx,
                                       p->bat.icost, d_qi.get(), (double *)nullptr);
                if (p->ic_ld > n)
                    hipLaunchKernelGGL(k_inst_const, dim3((batch + 3) / 4), dim3(256), 0, sq, batch, n, nx, nW, p->ic_ld, p->bat.icost, p->bat.x0, p->bat.omega, d_rc.get());
            }
            hipLaunchKernelGGL(k_eval_obj, dim3(batch), dim3(256), sizeof(double) * std::max(1, n), sq, n, nx, nW, p->d_q0.get(), inst_q ? d_qi.get() : nullptr,
                               p->has_quad ? p->d_P.get() : nullptr, nx ? p->d_cx.get() : nullptr, nW ? p->d_cw.get() : nullptr, p->d_c0.get(),
                               inst_q ? d_rc.get() : nullptr, midx, pv, p->bat.x0.get(), p->bat.omega.get(), st, ob, d_obj.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(obj_out, d_obj, sizeof(double) * batch, hipMemcpyDeviceToHost, sq));
        }
        return MLD_OK;
    };
    rc = queue();
    const hipError_t es = hipStreamSynchronize(sq);
    if (rc) return rc;
    HIP_TRY(es);
    return MLD_OK;
}

int mld_evaluate_batch(mld_problem_t *p, const double *v, int n_cols, const double *omega_cols, const int32_t *col_rows, const double *x_cols,
                       double *obj_out, double *constr_vio_out, int32_t *constr_row_out, double *int_vio_out, double *bound_vio_out)
{
    return evaluate_impl(p, "mld_evaluate_batch", v, n_cols, omega_cols, false, nullptr, 0, col_rows, x_cols, obj_out, constr_vio_out, constr_row_out, int_vio_out, bound_vio_out);
}

int mld_evaluate_batch_profiles(mld_problem_t *p, const double *v, int n_cols, const int64_t *start, int step, const int32_t *col_rows, const double *x_cols,
                                double *obj_out, double *constr_vio_out, int32_t *constr_row_out, double *int_vio_out, double *bound_vio_out)
{
    return evaluate_impl(p, "mld_evaluate_batch_profiles", v, n_cols, nullptr, true, start, step, col_rows, x_cols, obj_out, constr_vio_out, constr_row_out, int_vio_out, bound_vio_out);
}

/* ---- plant step and simulation log of the resident batch -------------------------------------------------------------------------------------------
 * One step of the reference's closed loop after the solve: ControllerBase.sim_step_k -> MldModel.lsim_k -> MldSimLog (controllers/controller_base.py:
 * 229-253, models/mld_model.py:647-699, controller_base.py:58-146), with the whole step-0 slice v0 = [u; delta; z; mu] given (lsim_k's v_k=, no
 * auxiliary resolution) -- the resident plan's or the caller's -- under the forecast's step 0 or the REALISED disturbance out of the profile library.
 * Kernel: sim_step.inc.  Everything is tested on the host before anything is queued, the new inputs are built in the spare buffers and swapped in by
 * the host, the starts of the realised series in a buffer of their own: a call that is refused changes nothing. */
int mld_sim_log_begin(mld_problem_t *p, int capacity)
{
    static const char who[] = "mld_sim_log_begin";
    if (mld_device_count() <= 0) { mld_set_error("no HIP device (libmldgpu has no CPU fallback)"); return MLD_ERR_NO_DEVICE; }
    MLD_NOT_IN_FLIGHT(p, who);
    if (!p || p->batch < 1) { mld_set_error("%s: no batch resident (mld_upload_batch): the log belongs to a batch", who); return MLD_ERR_INVALID; }
    if (capacity < 0) { mld_set_error("%s: capacity = %d", who, capacity); return MLD_ERR_INVALID; }
    if (capacity == 0) { p->slog = mld_problem::SimLog(); return MLD_OK; }
    const mld_dims &d = p->model->dims;
    const size_t widest = (size_t)std::max(std::max(std::max(d.nx, p->nv), std::max(d.ny, d.nomega)), std::max(d.nc, 1));
    const size_t cb = (size_t)capacity * (size_t)p->batch;
    if (cb > SIZE_MAX / sizeof(double) / widest) { mld_set_error("%s: capacity %d x batch %d x %zu entries does not fit size_t", who, capacity, p->batch, widest); return MLD_ERR_INVALID; }
    mld_problem::SimLog L;      /* built beside the resident log: an allocation failure leaves that as it was */
    hipError_t e = hipSuccess;
    auto take = [&](auto &buf, size_t count) { if (e == hipSuccess) e = buf.alloc(count); };
    take(L.x, cb * d.nx); take(L.v, cb * p->nv); take(L.y, cb * d.ny); take(L.om, cb * d.nomega); take(L.x_k1, cb * d.nx);
    take(L.vio, cb); take(L.obj, cb); take(L.lb, cb); take(L.cons, cb * d.nc); take(L.row, cb); take(L.status, cb); take(L.nodes, cb);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        mld_set_error("%s: %s for %d records of %d instances (%zu bytes)", who, hipGetErrorString(e), capacity, p->batch,
                      cb * ((2 * (size_t)d.nx + p->nv + d.ny + d.nomega + 3) * sizeof(double) + d.nc + 3 * sizeof(int)));
        return MLD_ERR_HIP;
    }
    L.cap = capacity; L.count = 0;
    p->slog = std::move(L);
    return MLD_OK;
}

int mld_sim_log_count(mld_problem_t *p, int32_t *n_logged, int32_t *capacity)
{
    if (!p) { mld_set_error("mld_sim_log_count: null problem"); return MLD_ERR_INVALID; }
    if (n_logged) *n_logged = p->slog.count;
    if (capacity) *capacity = p->slog.cap;
    return MLD_OK;
}

int mld_sim_step_batch(mld_problem_t *p, const double *v0, const int64_t *act_start, int step, int flags,
                       double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out, int32_t *n_skipped_out)
{
    static const char who[] = "mld_sim_step_batch";
    if (mld_device_count() <= 0) { mld_set_error("no HIP device (libmldgpu has no CPU fallback)"); return MLD_ERR_NO_DEVICE; }
    MLD_NOT_IN_FLIGHT(p, who);
    if (!p || p->batch < 1) { mld_set_error("%s: no batch resident (mld_upload_batch)", who); return MLD_ERR_INVALID; }
    mld_model *m = p->model;
    const mld_dims &d = m->dims;
    const int batch = p->batch, nx = d.nx, nv = p->nv, nw = d.nomega, ny = d.ny, nc = d.nc;
    if (flags & ~(MLD_SIM_ADVANCE | MLD_SIM_ACTUAL | MLD_SIM_LOG)) { mld_set_error("%s: unknown flag bits 0x%x (MLD_SIM_ADVANCE | MLD_SIM_ACTUAL | MLD_SIM_LOG)", who, flags); return MLD_ERR_INVALID; }
    const bool advance = flags & MLD_SIM_ADVANCE, actual = flags & MLD_SIM_ACTUAL, log = flags & MLD_SIM_LOG;
    if (step < 0 || step == INT_MAX) { mld_set_error("%s: step = %d (must be >= 0)", who, step); return MLD_ERR_INVALID; }
    if (m->tv_N > 0) { mld_set_error("%s: time-varying models (mld_model_create_tv) are not stepped on the device -- the step models would have to shift with the horizon (as mld_advance_batch)", who); return MLD_ERR_INVALID; }
    if (!m->d_pack) { mld_set_error("%s: model without matrices", who); return MLD_ERR_INVALID; }
    if (!v0 && !p->solved) { mld_set_error("%s: the resident batch has not been solved since its upload / selection (there is no plan to apply; pass v0)", who); return MLD_ERR_INVALID; }
    if (!v0 && p->advanced) { mld_set_error("%s: the last solve's plan has already been applied -- the resident plan belongs to inputs that are gone (solve again, or pass v0)", who); return MLD_ERR_INVALID; }
    if (act_start && !actual) { mld_set_error("%s: act_start given without MLD_SIM_ACTUAL", who); return MLD_ERR_INVALID; }
    std::vector<long long> gmax;
    if (actual) {
        if (nw == 0) { mld_set_error("%s: MLD_SIM_ACTUAL, but the model has no disturbance (nomega = 0)", who); return MLD_ERR_INVALID; }
        if (!p->pf_len) { mld_set_error("%s: MLD_SIM_ACTUAL, but no profile library is resident (mld_upload_profiles)", who); return MLD_ERR_INVALID; }
        /* the window rule with ONE step: s >= 0 and s + (step + 1) * width_g <= lib_len */
        if (act_start) {
            gmax.assign(p->pf_groups, 0);
            const int64_t *s = act_start;
            for (int b = 0; b < batch; ++b)
                for (int g = 0; g < p->pf_groups; ++g, ++s) {
                    if (!profile_start_ok(*s, p->pf_len, step, 1, p->pf_width[g])) {
                        mld_set_error("%s: actual start %lld of instance %d, group %d (width %d) at step %d: the element [%lld, %lld) leaves the library of %lld doubles",
                                      who, (long long)*s, b, g, p->pf_width[g], step, (long long)*s + (long long)step * p->pf_width[g],
                                      (long long)*s + ((long long)step + 1) * p->pf_width[g], p->pf_len);
                        return MLD_ERR_INVALID;
                    }
                    gmax[g] = std::max<long long>(gmax[g], *s);
                }
        } else {
            if (p->pf_abatch != batch) { mld_set_error("%s: act_start == NULL, but no actual starts of this batch are resident (pass them once)", who); return MLD_ERR_INVALID; }
            for (int g = 0; g < p->pf_groups; ++g)
                if (!profile_start_ok(p->pf_amax[g], p->pf_len, step, 1, p->pf_width[g])) {
                    mld_set_error("%s: step %d moves the largest resident actual start of group %d (%lld, width %d) past the end of the library: the element would end at %lld of %lld doubles",
                                  who, step, g, p->pf_amax[g], p->pf_width[g], p->pf_amax[g] + ((long long)step + 1) * p->pf_width[g], p->pf_len);
                    return MLD_ERR_INVALID;
                }
        }
    }
    mld_problem::SimLog &L = p->slog;
    if (log && !L.cap) { mld_set_error("%s: MLD_SIM_LOG, but no log has been begun for this batch (mld_sim_log_begin)", who); return MLD_ERR_INVALID; }
    if (log && L.count >= L.cap) { mld_set_error("%s: MLD_SIM_LOG, but the log is full (%d of %d records; mld_download_sim_log, then mld_sim_log_begin)", who, L.count, L.cap); return MLD_ERR_INVALID; }
    if (!advance && !log && !x_k1_out && !y_out && !cons_out && !cons_vio_out && !cons_row_out && !n_skipped_out && !act_start) return MLD_OK;      /* nothing asked for */

    SimStepArgs a{};
    a.batch = batch; a.nx = nx; a.nv = nv; a.nmu = d.nmu; a.nw = nw; a.ny = ny; a.nc = nc; a.N = p->N;
    const size_t stage = sizeof(double) * SS_WAVES * ((size_t)nx + nv + nw + ny);
    a.lds = stage <= SS_LDS_MAX && !(p->opts.reserved & MLD_DBG_SIM_NO_LDS);
    a.pack = m->d_pack; a.pack_len = m->pack_len;
    {   /* offsets inside the packed per-model block: A, B4, b5, C, D4, d5, E, F4, f5, G, [B1 B2 B3 0], [D1 D2 D3 0], [F1 F2 F3 Psi]  (mld_model_create) */
        size_t o = 0;
        a.oA = o; o += m->mat_size[MT_A]; a.oB4 = o; o += m->mat_size[MT_B4]; a.ob5 = o; o += m->mat_size[MT_b5];
        a.oC = o; o += m->mat_size[MT_C]; a.oD4 = o; o += m->mat_size[MT_D4]; a.od5 = o; o += m->mat_size[MT_d5];
        a.oE = o; o += m->mat_size[MT_E]; a.oF4 = o; o += m->mat_size[MT_F4]; a.of5 = o; o += m->mat_size[MT_f5];
        a.oG = o; o += m->mat_size[MT_G];
        a.oBv = o; o += (size_t)nx * nv; a.oDv = o; o += (size_t)ny * nv; a.oFv = o;
    }
    a.model_idx = p->has_midx ? p->bat.model_idx.get() : nullptr;
    a.x0 = p->bat.x0; a.omega = p->bat.omega;
    const hipStream_t sq = p->stream;
    DevBuf<double> d_v, d_xk1, d_y, d_vio; DevBuf<unsigned char> d_cons; DevBuf<int> d_row; DevBuf<long long> d_start;
    if (v0) HIP_TRY(d_v.alloc((size_t)batch * std::max(1, nv)));
    if (act_start) HIP_TRY(d_start.alloc((size_t)batch * p->pf_groups));
    if (!a.lds && !p->bat.sim_tmp) HIP_TRY(p->bat.sim_tmp.alloc((size_t)p->in_cap * std::max(1, nw + ny)));      /* sized like the input buffers (any batch up to in_cap); free_batch releases it with them */
    if (!a.lds) { a.w_tmp = p->bat.sim_tmp; a.y_tmp = p->bat.sim_tmp.get() + (size_t)batch * nw; }
    if (v0) { a.v = d_v; a.v_stride = (size_t)nv; }
    else {      /* the resident plans: rows < batch are the instances' (after the hand-off's device merge), hand-off items come after them */
        a.v = p->bat.v; a.v_stride = (size_t)p->n;
        a.status = p->bat.status; a.obj = p->bat.obj; a.lbnd = p->bat.lbnd; a.nodes = p->bat.nodes;
    }
    if (actual) { a.act_start = act_start ? d_start.get() : p->pf_astart.get(); a.chan = p->pf_chan; a.n_groups = p->pf_groups; a.step = step; a.lib = p->pf_lib; }
    if (advance) { a.x0_new = p->bat.x0b; a.omega_new = p->bat.omegab; }
    const size_t slot = log ? (size_t)L.count * batch : 0;
    if (log) {
        a.x_k1 = L.x_k1.get() + slot * nx; a.y = L.y.get() + slot * ny; a.vio = L.vio.get() + slot; a.cons = L.cons.get() + slot * nc; a.row = L.row.get() + slot;
        a.rec_x = L.x.get() + slot * nx; a.rec_v = L.v.get() + slot * nv; a.rec_om = L.om.get() + slot * nw;
        a.rec_obj = L.obj.get() + slot; a.rec_lb = L.lb.get() + slot; a.rec_status = L.status.get() + slot; a.rec_nodes = L.nodes.get() + slot;
    } else {
        if (x_k1_out && nx) { HIP_TRY(d_xk1.alloc((size_t)batch * nx)); a.x_k1 = d_xk1; }
        if (y_out && ny) { HIP_TRY(d_y.alloc((size_t)batch * ny)); a.y = d_y; }
        if (cons_out && nc) { HIP_TRY(d_cons.alloc((size_t)batch * nc)); a.cons = d_cons; }
        if (cons_vio_out) { HIP_TRY(d_vio.alloc(batch)); a.vio = d_vio; }
        if (cons_row_out) { HIP_TRY(d_row.alloc(batch)); a.row = d_row; }
    }
    const bool count_skipped = !v0 && (n_skipped_out != nullptr);
    if (count_skipped) a.n_skipped = p->bat.skipped;
    int skipped = 0;
    /* the host waits where it has to: for the caller's arrays (theirs again when this returns), the skip count and the requested outputs; and after an
     * advance on a stream of the problem's own, because the other entry points copy on the legacy stream, which does not order against that one */
    const bool wait = v0 || act_start || count_skipped || x_k1_out || y_out || cons_out || cons_vio_out || cons_row_out || (advance && p->own_stream);
    auto queue = [&]() -> int {
        if (v0 && nv) HIP_TRY(hipMemcpyAsync(d_v, v0, sizeof(double) * (size_t)batch * nv, hipMemcpyHostToDevice, sq));
        if (act_start) HIP_TRY(hipMemcpyAsync(d_start, act_start, sizeof(long long) * (size_t)batch * p->pf_groups, hipMemcpyHostToDevice, sq));
        if (count_skipped) HIP_TRY(hipMemsetAsync(p->bat.skipped, 0, sizeof(int), sq));
        const int grid = (int)std::min<long long>(((long long)batch + SS_WAVES - 1) / SS_WAVES, 8192);
        hipLaunchKernelGGL(k_sim_step, dim3(grid), dim3(64 * SS_WAVES), a.lds ? stage : 0, sq, a);
        HIP_TRY(hipGetLastError());
        if (x_k1_out && nx) HIP_TRY(hipMemcpyAsync(x_k1_out, a.x_k1, sizeof(double) * (size_t)batch * nx, hipMemcpyDeviceToHost, sq));
        if (y_out && ny) HIP_TRY(hipMemcpyAsync(y_out, a.y, sizeof(double) * (size_t)batch * ny, hipMemcpyDeviceToHost, sq));
        if (cons_out && nc) HIP_TRY(hipMemcpyAsync(cons_out, a.cons, (size_t)batch * nc, hipMemcpyDeviceToHost, sq));
        if (cons_vio_out) HIP_TRY(hipMemcpyAsync(cons_vio_out, a.vio, sizeof(double) * batch, hipMemcpyDeviceToHost, sq));
        if (cons_row_out) HIP_TRY(hipMemcpyAsync(cons_row_out, a.row, sizeof(int) * batch, hipMemcpyDeviceToHost, sq));
        if (count_skipped) HIP_TRY(hipMemcpyAsync(&skipped, p->bat.skipped, sizeof(int), hipMemcpyDeviceToHost, sq));
        return MLD_OK;
    };
    const int rc = queue();
    if (rc || wait) {
        const hipError_t es = hipStreamSynchronize(sq);
        if (rc) return rc;
        HIP_TRY(es);
    }
    /* queued without an error: the handle moves on */
    if (act_start) { p->pf_astart = std::move(d_start); p->pf_abatch = batch; p->pf_amax = gmax; }
    if (log) ++L.count;
    if (advance) {
        std::swap(p->bat.x0, p->bat.x0b); std::swap(p->bat.omega, p->bat.omegab);
        p->n_xcols = 0;      /* extra constraint blocks belonged to the previous step's data */
        p->has_warm = false; /* a start belongs to one set of inputs (mld_warm_start_from_previous builds the next one from the plan) */
        p->has_cutoff = false;
        if (v0) { p->solved = false; p->advanced = false; }      /* the caller's inputs: new inputs, as after mld_select_inputs */
        else p->advanced = true;                                 /* the resident plan has been applied, as after mld_advance_batch */
    }
    if (n_skipped_out) *n_skipped_out = skipped;
    return MLD_OK;
}

int mld_download_sim_log(mld_problem_t *p, int first, int count, double *x, double *v, double *y, double *omega, double *x_k1, uint8_t *cons, double *cons_vio,
                         int32_t *cons_row, double *obj, double *lower_bound, int32_t *status, int32_t *nodes)
{
    static const char who[] = "mld_download_sim_log";
    if (mld_device_count() <= 0) { mld_set_error("no HIP device (libmldgpu has no CPU fallback)"); return MLD_ERR_NO_DEVICE; }
    MLD_NOT_IN_FLIGHT(p, who);
    if (!p || p->batch < 1) { mld_set_error("%s: no batch resident (mld_upload_batch)", who); return MLD_ERR_INVALID; }
    const mld_problem::SimLog &L = p->slog;
    if (first < 0 || count < 0 || (long long)first + count > L.count) { mld_set_error("%s: records [%d, %lld) asked for, %d logged", who, first, (long long)first + count, L.count); return MLD_ERR_INVALID; }
    if (count == 0) return MLD_OK;
    const mld_dims &d = p->model->dims;
    const size_t off = (size_t)first * p->batch, len = (size_t)count * p->batch;
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int {
        auto get = [&](void *dst, const void *src, size_t width, size_t elem) -> hipError_t {
            if (!dst || !width) return hipSuccess;
            return hipMemcpyAsync(dst, (const char *)src + off * width * elem, len * width * elem, hipMemcpyDeviceToHost, sq);
        };
        HIP_TRY(get(x, L.x.get(), d.nx, sizeof(double))); HIP_TRY(get(v, L.v.get(), p->nv, sizeof(double))); HIP_TRY(get(y, L.y.get(), d.ny, sizeof(double)));
        HIP_TRY(get(omega, L.om.get(), d.nomega, sizeof(double))); HIP_TRY(get(x_k1, L.x_k1.get(), d.nx, sizeof(double))); HIP_TRY(get(cons, L.cons.get(), d.nc, 1));
        HIP_TRY(get(cons_vio, L.vio.get(), 1, sizeof(double))); HIP_TRY(get(cons_row, L.row.get(), 1, sizeof(int)));
        HIP_TRY(get(obj, L.obj.get(), 1, sizeof(double))); HIP_TRY(get(lower_bound, L.lb.get(), 1, sizeof(double)));
        HIP_TRY(get(status, L.status.get(), 1, sizeof(int))); HIP_TRY(get(nodes, L.nodes.get(), 1, sizeof(int)));
        return MLD_OK;
    };
    const int rc = queue();
    const hipError_t es = hipStreamSynchronize(sq);
    if (rc) return rc;
    HIP_TRY(es);
    return MLD_OK;
}

int mld_problem_get_opts(mld_problem_t *p, mld_opts *out)
{
    if (!p || !out) { mld_set_error("mld_problem_get_opts: bad arguments"); return MLD_ERR_INVALID; }
    *out = p->opts;      /* with every size-scaled default resolved */
    out->n_slots = p->n_slots;
    return MLD_OK;
}

int mld_problem_set_opts(mld_problem_t *p, const mld_opts *o)
{
    MLD_NOT_IN_FLIGHT(p, "mld_problem_set_opts");
    if (!p || !o) { mld_set_error("mld_problem_set_opts: bad arguments"); return MLD_ERR_INVALID; }
    /* limits and tolerances only: the workspace layout (max_cuts, n_slots) and the tightened model (presolve) stay.  Every check comes BEFORE the first
     * assignment: a refused call changes nothing (ADVICE r3). */
    if (o->flags != p->opts.flags) { mld_set_error("mld_problem_set_opts: flags (MLD_F32) are fixed at mld_problem_create -- they decide how the cost is assembled"); return MLD_ERR_INVALID; }
    if (!(o->gap_abs >= 0.0) || !(o->gap_rel >= 0.0) || o->max_nodes < 1 || o->max_pivots < 1) { mld_set_error("mld_problem_set_opts: gaps must be >= 0, node / pivot limits >= 1"); return MLD_ERR_INVALID; }
    p->opts.gap_abs = o->gap_abs; p->opts.gap_rel = o->gap_rel; p->opts.max_nodes = o->max_nodes; p->opts.max_pivots = o->max_pivots;
    p->opts.reserved = o->reserved;
    if (o->time_limit >= 0.0) p->opts.time_limit = o->time_limit;      /* (negative keeps the current value) */
    if (o->cut_rounds >= 0) p->opts.cut_rounds = p->opts.max_cuts > 0 ? o->cut_rounds : 0;
    if (o->cuts_per_round >= 0) p->opts.cuts_per_round = o->cuts_per_round;
    if (o->mir_per_round >= 0) p->opts.mir_per_round = o->mir_per_round;
    SolverShape &S = p->S;
    S.cuts_per_round = p->opts.cuts_per_round; S.cut_rounds = p->opts.cut_rounds; S.mir_per_round = p->opts.mir_per_round;
    S.max_nodes = p->opts.max_nodes; S.max_pivots = p->opts.max_pivots; S.gap_abs = p->opts.gap_abs; S.gap_rel = p->opts.gap_rel;
    S.debug = p->opts.reserved; S.time_ticks = time_limit_ticks(p->opts.time_limit);
    return MLD_OK;
}

int mld_solve_batch(mld_problem_t *p, int batch, const int32_t *model_idx, const double *x0, const double *omega,
                    const uint8_t *fixed_bin, double *v_out, double *obj_out, int32_t *status_out,
                    double *lower_bound_out, mld_stats *stats_out)
{
    int rc = mld_upload_batch(p, batch, model_idx, x0, omega, fixed_bin);
    if (rc) return rc;
    if ((rc = mld_solve_resident(p, stats_out))) return rc;
    return mld_download_results(p, v_out, obj_out, status_out, lower_bound_out, nullptr, nullptr);
}

int mld_rhs_batch(mld_problem_t *p, int batch, int scenarios, const int32_t *model_idx, const double *x0,
                  const double *omega, double *h_out)
{
    if (!p || batch < 1 || scenarios < 1 || !h_out) { mld_set_error("mld_rhs_batch: bad arguments"); return MLD_ERR_INVALID; }
    if ((p->nx && !x0) || (p->nW && !omega)) { mld_set_error("mld_rhs_batch: x0/omega required"); return MLD_ERR_INVALID; }
    if (model_idx) for (int k = 0; k < batch; ++k) if (model_idx[k] < 0 || model_idx[k] >= p->n_models) { mld_set_error("model_idx[%d]=%d out of range", k, model_idx[k]); return MLD_ERR_INVALID; }
    mld_model *m = p->model;
    int rc;
    if (m->cond_N != p->N && (rc = condense_model_device(m, p->N, nullptr, 0))) return rc;
    /* temporaries of this call: released on every return path (HIP_TRY returns early) */
    DevBuf<int> d_idx, d_perm; DevBuf<double> d_x, d_w, d_h; DevBuf<RhsGroup> d_groups;
    const size_t b = batch;
    if (model_idx) { HIP_TRY(d_idx.alloc(b)); HIP_TRY(hipMemcpy(d_idx, model_idx, sizeof(int) * b, hipMemcpyHostToDevice)); }
    HIP_TRY(d_x.alloc(b * std::max(1, p->nx)));
    HIP_TRY(d_w.alloc(b * scenarios * std::max(1, p->nW)));
    HIP_TRY(d_h.alloc(b * std::max(1, p->m0)));
    if (p->nx) HIP_TRY(hipMemcpy(d_x, x0, sizeof(double) * b * p->nx, hipMemcpyHostToDevice));
    if (p->nW) HIP_TRY(hipMemcpy(d_w, omega, sizeof(double) * b * scenarios * p->nW, hipMemcpyHostToDevice));
    if (p->m0 && scenarios == 1 && rhs_mfma_fits(p->nx, p->nW) && !(p->opts.reserved & MLD_DBG_GEMM_VALU)) {
        std::vector<int> perm; std::vector<RhsGroup> groups;
        build_rhs_groups(model_idx, batch, p->n_models, perm, groups);
        if (!perm.empty()) { HIP_TRY(d_perm.alloc(perm.size())); HIP_TRY(hipMemcpy(d_perm, perm.data(), sizeof(int) * perm.size(), hipMemcpyHostToDevice)); }
        HIP_TRY(d_groups.alloc(groups.size()));
        HIP_TRY(hipMemcpy(d_groups, groups.data(), sizeof(RhsGroup) * groups.size(), hipMemcpyHostToDevice));
        launch_rhs_mfma((p->opts.flags & MLD_F32) != 0, (int)groups.size(), p->m0, p->nx, p->nW, m->d_out[O_HX], m->d_out[O_HW], m->d_out[O_H5],
                        (const double *)nullptr, d_groups, d_perm, d_x, d_w, d_h);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(h_out, d_h, sizeof(double) * b * p->m0, hipMemcpyDeviceToHost));
    } else if (p->m0) {
        hipLaunchKernelGGL(k_rhs, dim3(batch), dim3(256), 0, 0, p->m0, p->nx, p->nW, m->d_out[O_HX], m->d_out[O_HW], m->d_out[O_H5],
                           (const double *)nullptr, d_idx, d_x, d_w, d_h, scenarios);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(h_out, d_h, sizeof(double) * b * p->m0, hipMemcpyDeviceToHost));
    }
    return MLD_OK;
}

// ---- RCCL gather ---------------------------------------------------------------------------------
static ncclComm_t g_comm = nullptr;
static int g_nranks = 0;

int mld_comm_unique_id(uint8_t id[MLD_COMM_ID_BYTES])
{
    static_assert(sizeof(ncclUniqueId) <= MLD_COMM_ID_BYTES, "id size");
    ncclUniqueId u;
    ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) { mld_set_error("ncclGetUniqueId: %s", ncclGetErrorString(r)); return MLD_ERR_COMM; }
    memset(id, 0, MLD_COMM_ID_BYTES);
    memcpy(id, &u, sizeof(u));
    return MLD_OK;
}

int mld_comm_init(int n_ranks, int rank, const uint8_t id[MLD_COMM_ID_BYTES])
{
    if (mld_device_count() <= 0) { mld_set_error("no HIP device"); return MLD_ERR_NO_DEVICE; }
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclResult_t r = ncclCommInitRank(&g_comm, n_ranks, u, rank);
    if (r != ncclSuccess) { mld_set_error("ncclCommInitRank: %s", ncclGetErrorString(r)); return MLD_ERR_COMM; }
    g_nranks = n_ranks;
    return MLD_OK;
}

int mld_gather(const double *send, int count, double *recv)
{
    if (!g_comm) { mld_set_error("mld_gather: communicator not initialised"); return MLD_ERR_COMM; }
    DevBuf<double> d_s, d_r;
    HIP_TRY(d_s.alloc(std::max(1, count)));
    HIP_TRY(d_r.alloc((size_t)std::max(1, count) * g_nranks));
    hipError_t e = hipMemcpy(d_s, send, sizeof(double) * count, hipMemcpyHostToDevice);
    ncclResult_t r = ncclSuccess;
    if (e == hipSuccess) r = ncclAllGather(d_s, d_r, count, ncclDouble, g_comm, 0);
    if (e == hipSuccess && r == ncclSuccess) e = hipStreamSynchronize(0);
    if (e == hipSuccess && r == ncclSuccess) e = hipMemcpy(recv, d_r, sizeof(double) * count * g_nranks, hipMemcpyDeviceToHost);
    if (r != ncclSuccess) { mld_set_error("ncclAllGather: %s", ncclGetErrorString(r)); return MLD_ERR_COMM; }
    if (e != hipSuccess) { mld_set_error("mld_gather: %s", hipGetErrorString(e)); return MLD_ERR_HIP; }
    return MLD_OK;
}

} // extern "C"

// send[b] = (objective, status, step-0 slice of v) of the solved batch, packed on device for the all-gather
__global__ void __launch_bounds__(256) k_pack_results(int batch, int n, int nv, const double *obj, const int *status, const double *v, double *send)
{
    const int w = 2 + nv;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)batch * w; e += (size_t)gridDim.x * blockDim.x) {
        const size_t b = e / w; const int c = (int)(e % w);
        send[e] = c == 0 ? obj[b] : (c == 1 ? (double)status[b] : v[b * n + (c - 2)]);
    }
}

extern "C" int mld_gather_results(mld_problem_t *p, double *recv, int *width_out)
{
    if (!g_comm) { mld_set_error("mld_gather_results: communicator not initialised"); return MLD_ERR_COMM; }
    if (!p || p->batch < 1 || !recv) { mld_set_error("mld_gather_results: nothing solved"); return MLD_ERR_INVALID; }
    MLD_NOT_IN_FLIGHT(p, "mld_gather_results");
    const int w = 2 + p->nv;
    const size_t count = (size_t)p->batch * w;
    /* send / receive buffers live with the problem (a hipFree per call synchronises the whole device: with two handles in flight the gather of
     * one would wait for the other's solve), and pack + all-gather run on the problem's own stream */
    if (p->gather_cap < count * (size_t)(1 + g_nranks)) {
        p->gather_cap = 0;
        HIP_TRY(p->d_gather.alloc(count * (size_t)(1 + g_nranks)));
        p->gather_cap = count * (size_t)(1 + g_nranks);
    }
    double *d_s = p->d_gather, *d_r = p->d_gather + count;
    const hipStream_t sq = p->stream;
    hipLaunchKernelGGL(k_pack_results, dim3((unsigned)std::min<size_t>((count + 255) / 256, 65535)), dim3(256), 0, sq, p->batch, p->n, p->nv, p->bat.obj, p->bat.status, p->bat.v, d_s);
    hipError_t e = hipGetLastError();
    ncclResult_t r = e == hipSuccess ? ncclAllGather(d_s, d_r, count, ncclDouble, g_comm, sq) : ncclSuccess;
    if (r == ncclSuccess && e == hipSuccess) e = hipMemcpyAsync(recv, d_r, sizeof(double) * count * g_nranks, hipMemcpyDeviceToHost, sq);
    if (r == ncclSuccess && e == hipSuccess) e = hipStreamSynchronize(sq);
    if (r != ncclSuccess) { mld_set_error("ncclAllGather: %s", ncclGetErrorString(r)); return MLD_ERR_COMM; }
    if (e != hipSuccess) { mld_set_error("mld_gather_results: %s", hipGetErrorString(e)); return MLD_ERR_HIP; }
    if (width_out) *width_out = w;
    return MLD_OK;
}

extern "C" int mld_comm_destroy(void)
{
    if (g_comm) { ncclCommDestroy(g_comm); g_comm = nullptr; }
    return MLD_OK;
}
