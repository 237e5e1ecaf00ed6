// Small kernels of the problem handle: cost assembly (K4), receding horizon, MIP start, fills and statistics, result packing.
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

__global__ void __launch_bounds__(256) k_advance(int batch, int nx, int nv, int nw, int N, const double *pack, size_t pack_len, PackOff off,
                                                const int *model_idx, const double *x0, const double *omega, const double *v, size_t v_stride,
                                                double *x0_new, double *omega_new, const int *status, const double *obj, int *n_skipped)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nW = (size_t)N * nw;
    if (t < (size_t)batch && !plan_usable(status, obj, (int)t)) atomicAdd(n_skipped, 1);
    if (t < (size_t)batch * nx) {
        const int b = (int)(t / nx), i = (int)(t % nx);
        if (!plan_usable(status, obj, b)) { x0_new[t] = x0[t]; }      // no plan: the plant of this instance is not advanced
        else {
        const double *pk = pack + (size_t)(model_idx ? model_idx[b] : 0) * pack_len;
        const double *xb = x0 + (size_t)b * nx, *wb = omega + (size_t)b * nW, *vb = v + (size_t)b * v_stride;
        x0_new[t] = plant_row(i, pk + off.b5, pk + off.A, pk + off.Bv, pk + off.B4, nx, nv, nw, xb, vb, wb);
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

// MIP start from a rollout (mld_warm_start_from_rollout): binary k of instance b takes the rounded value of its per-step variable in the rolled-out
// trajectory's v (batch, N_tilde, nv), a device temporary; an instance whose trajectory did not end complete gets none (the whole row 255), one that keeps
// its resident start is not written.  Threads on (instance, binary), a 64-bit flat index; the thread of an instance's binary 0 writes its source.  The rule
// of one element is ws_element (warm_rollout.inc).
#include "warm_rollout.inc"
__global__ void __launch_bounds__(256) k_warm_from_rollout(long long batch, int nb, int nv, const int *bins, const double *v, size_t v_stride, const int *end_status,
                                                          const unsigned char *old, unsigned char *warm, int *source)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (unsigned long long)batch * (unsigned)nb) return;
    const int src = ws_element(t, nb, nv, bins, v, v_stride, end_status, old, warm);
    if (t % (unsigned)nb == 0) source[t / (unsigned)nb] = src;
}

#include "trajectory.inc"      // k_trajectory / k_trajectory_valu (mld_predict_batch): they mask with plan_usable, like k_advance
#include "evaluate.inc"        // k_evaluate / k_evaluate_valu, k_eval_point, k_eval_obj (mld_evaluate_batch): the same masking
#include "sim_step.inc"        // k_sim_step (mld_sim_step_batch): lsim_k with the whole step-0 slice, the same masking
#include "aux_step.inc"        // k_aux_inputs / k_aux_merge (mld_sim_step_resolve): between a handle and its auxiliary resolver, the same masking
#include "rollout.inc"         // k_rollout (mld_rollout_batch): K resolved steps per trajectory in one wave, the same masking
#include "rollout_risk.inc"    // k_rollout_risk (mld_rollout_risk): statistics across a rollout's realisations, a wave per instance
#include "plan_select.inc"     // k_plan_select (mld_rollout_select): the admissible candidate plan of least objective statistic, a wave per instance
#include "fallback.inc"        // k_fallback_inputs / k_fallback_commit (mld_sim_step_fallback): the source of u for an instance without a usable plan
#include "selected.inc"        // k_selected_inputs / k_selected_commit (mld_sim_step_selected): a kept selection as the first source of u

// out[k] = a[k] * b[k]
__global__ void __launch_bounds__(256) k_scale_vec(size_t count, const double *a, const double *b, double *out)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) out[k] = a[k] * b[k];
}

/* (C linkage, as they have always had: the names are part of the code object and of the library's symbol list) */
extern "C" {
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
}

// send[b] = (objective, status, step-0 slice of v) of the solved batch, packed on device for the all-gather
__global__ void __launch_bounds__(256) k_pack_results(int batch, int n, int nv, const double *obj, const int *status, const double *v, double *send)
{
    const int w = 2 + nv;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)batch * w; e += (size_t)gridDim.x * blockDim.x) {
        const size_t b = e / w; const int c = (int)(e % w);
        send[e] = c == 0 ? obj[b] : (c == 1 ? (double)status[b] : v[b * n + (c - 2)]);
    }
}
