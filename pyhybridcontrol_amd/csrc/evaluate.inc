// Solution quality of a resident batch (mld_evaluate_batch): what the reference's backend reports after every solve (ObjVal, ConstrVio, IntVio,
// BoundVio; controllers/controller_base.py:509) for any plans, against the ORIGINAL condensed rows and any set of disturbance columns
// (the column layout of gen_evo_constraints, controller_base.py:411-456).  The residual of row i of instance b under column c is
//     r_i = (H_v v_b)_i - (H_x x_c + H_omega omega_c + H_5)_i                       unscaled; negative = slack
// and the kernel keeps max_i r_i and a row that attains it.  A member of the instance-GEMM family (mfma.inc), with row tiles (ig_stage).  What it
// adds: two products in one launch, the causal skip below, and an epilogue that keeps a running (max, row) instead of storing residuals.  Always
// fp64 (a certificate in fp32 certifies nothing), also on a handle created with MLD_F32.
//
// Two passes in ONE launch, both with the inner dimension in chunks of IG_KC whose A fragments live in registers:
//   pass V   hv[b, i] = (H_v v_b)_i, chunk by chunk over n (cfg4: 575 = 3 chunks) -- the part every column shares, computed once.  Like k_trajectory
//            the accumulator is global memory, written by the first chunk and read and written by the same lane in every later one.
//   pass C   per column c: (H_x x_c + H_omega omega_c)_i, normally ONE chunk (cfg4: 207), so the residual hv - that - H_5 is complete in the lane
//            that holds the product: the epilogue stores nothing per row, it keeps a running (max, row) for the lane's four instances, which is
//            reduced across the 16 lanes that share an instance and written once per (instance, column).  Where nx + N nw > IG_KC the partial
//            products go through `part` (same lane reads what it wrote) and the last chunk reduces.
// The lane that owns (instance, row) is the same in both passes, so no synchronisation is needed between them.
//
// Causal skip: block (i, j) of H_v and H_omega is zero for j > i (the rows of step i see the inputs of steps <= i;
// tests/test_quality_host.py pins this on the condensed maps, time-varying horizons included).  A 16-row block whose last step is i reads the
// v / omega columns of steps j <= i only.  Groups of four inner indices are staged and multiplied whole: a group that straddles reads stored zeros.
#pragma once

struct EvCols {                      // the disturbance columns of one launch
    int n_cols;                      // columns of omc (after the standard one)
    int std;                         // 1: column 0 is the batch's own (x0, omega), all rows
    int per_col;                     // 1: one result per column (validation); 0: the maximum over all columns (the problem as posed)
    int ld_out;                      // per_col: results per instance in the output arrays (n_cols of the whole call); the launch writes col0 ..
    int col0;
    const double *x0, *omega;        // the batch's inputs (batch x nx, batch x nW)
    const double *omc;               // batch x n_cols x nW
    const double *xc;                // batch x n_cols x nx, or null = x0
    const int *rows;                 // n_cols leading rows each column applies to, or null = all
};

// (max, row) of the 16 lanes that share an instance (li = lane & 15), then one store by li == 0; dead instances get NaN / -1
__device__ __forceinline__ void ev_write(double (&best)[4], int (&brow)[4], const int (&oinst)[4], const bool (&dead)[4], int li, size_t ld, int col,
                                         double *vio, int *row_out)
{
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double b = best[r]; int w = brow[r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const double ob = __shfl_xor(b, o, 64); const int ow = __shfl_xor(w, o, 64);
            if (ob > b || (ob == b && ow >= 0 && (w < 0 || ow < w))) { b = ob; w = ow; }
        }
        if (li == 0 && oinst[r] >= 0) {
            if (vio) vio[(size_t)oinst[r] * ld + col] = dead[r] ? __builtin_nan("") : b;
            if (row_out) row_out[(size_t)oinst[r] * ld + col] = dead[r] ? -1 : w;
        }
    }
}

// Hv, Hx, Hw, H5: the original model's condensed rows (n_models x m0 x n / nx / nW / 1; Hx, Hw null when empty).  hv: batch x m0 scratch (pass V's
// result, kept between the launches of one call: do_v = 0 reuses it); part: batch x m0 scratch, needed only when nx + nW > IG_KC.
__global__ void __launch_bounds__(64 * RM_WAVES) k_evaluate(int m0, int nc, int nv, int nw, int n, int nx, int nW, const double *Hv, const double *Hx,
                                                            const double *Hw, const double *H5, const RhsGroup *groups, const int *perm, const double *v,
                                                            const int *status, const double *obj, int do_v, EvCols cols, double *hv, double *part,
                                                            double *vio, int *row_out)
{
    __shared__ double ev_tile[16 * IG_LD];
    const RhsGroup g = groups[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    int oinst[4]; bool dead[4];
    const int inst = ig_slots<false>(g, perm, wave, li, lk, oinst);
#pragma unroll
    for (int r = 0; r < 4; ++r) dead[r] = status && oinst[r] >= 0 && !plan_usable(status, obj, oinst[r]);
    const double *hvm = Hv ? Hv + (size_t)g.model * m0 * n : nullptr;
    const double *hxm = Hx ? Hx + (size_t)g.model * m0 * nx : nullptr, *hwm = Hw ? Hw + (size_t)g.model * m0 * nW : nullptr;
    const double *h5m = H5 + (size_t)g.model * m0;
    IgFrag<false, IG_KS> a;

    // ---- pass V: hv = H_v v ------------------------------------------------------------------------------------------------------------
    if (do_v) for (int kc0 = 0; kc0 < n || kc0 == 0; kc0 += IG_KC) {
        const int ks = (min(IG_KC, n - kc0) + 3) >> 2, g0 = kc0 >> 2;
        ig_load_a(a, inst, kc0, lk, ks, n, [=](int k) { return v[(size_t)inst * n + k]; });
        for (int rb = 0; rb < m0; rb += 16) {
            const int imax = min(rb + 15, m0 - 1) / nc;                          // the last step among the rows of this block
            const unsigned long long need = hvm ? ig_bits(-g0, ((min(n, (imax + 1) * nv) + 3) >> 2) - g0) & ig_bits(0, ks) : 0ull;
            if (!need && kc0 > 0) continue;                                      // nothing of this chunk reaches these rows (uniform over the workgroup)
            double res[4] = {0.0, 0.0, 0.0, 0.0};
            if (need) {
                ig_stage(ev_tile, tid, rb, kc0, need, [=](int row, int k) { return row < m0 && k < n ? hvm[(size_t)row * n + k] : 0.0; });
                ig_mma<4>(a, ev_tile + li * IG_LD + lk, IgMask{need}, res);               // B = H_v[rb + li][kc0 + k]
            }
            const int row = rb + li;
            if (row < m0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (oinst[r] < 0) continue;
                    double *dst = hv + (size_t)oinst[r] * m0 + row;
                    *dst = kc0 ? *dst + res[r] : res[r];
                }
            }
        }
    }

    // ---- pass C: per column, the right-hand side and the running maximum of the residual -----------------------------------------------------
    const int K2 = nx + nW, ncols = cols.std + cols.n_cols;
    const double ninf = -__builtin_huge_val();
    double best[4] = {ninf, ninf, ninf, ninf}; int brow_[4] = {-1, -1, -1, -1};
    for (int c = 0; c < ncols; ++c) {
        const bool own = cols.std && c == 0;
        const int j = c - cols.std;
        const int rows_c = own || !cols.rows ? m0 : min(cols.rows[j], m0);
        const double *xs = nullptr, *ws = nullptr;                              // this lane's instance under column c
        if (inst >= 0) {
            xs = own || !cols.xc ? cols.x0 + (size_t)inst * nx : cols.xc + ((size_t)inst * cols.n_cols + j) * nx;
            ws = own ? cols.omega + (size_t)inst * nW : cols.omc + ((size_t)inst * cols.n_cols + j) * nW;
        }
        if (cols.per_col) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { best[r] = ninf; brow_[r] = -1; }
        }
        for (int kc0 = 0; (kc0 < K2 || kc0 == 0) && rows_c > 0; kc0 += IG_KC) {
            const int ks = (min(IG_KC, K2 - kc0) + 3) >> 2, g0 = kc0 >> 2;
            const bool last = kc0 + IG_KC >= K2;
            ig_load_a(a, inst, kc0, lk, ks, K2, [=](int k) { return k < nx ? xs[k] : ws[k - nx]; });
            for (int rb = 0; rb < rows_c; rb += 16) {
                const int imax = min(rb + 15, m0 - 1) / nc;
                // (global groups [0, nx / 4 rounded up) of x -- H_x is dense -- and up to the last causal column of omega; a group that holds both is taken whole)
                unsigned long long need = 0ull;
                if (hxm) need |= ig_bits(-g0, ((nx + 3) >> 2) - g0);
                if (hwm) need |= ig_bits((nx >> 2) - g0, ((nx + min(nW, (imax + 1) * nw) + 3) >> 2) - g0);
                need &= ig_bits(0, ks);
                double prod[4] = {0.0, 0.0, 0.0, 0.0};
                if (need) {
                    ig_stage(ev_tile, tid, rb, kc0, need, [=](int row, int k) {
                        if (row >= m0 || k >= K2) return 0.0;
                        return k < nx ? (hxm ? hxm[(size_t)row * nx + k] : 0.0) : (hwm ? hwm[(size_t)row * nW + (k - nx)] : 0.0);
                    });
                    ig_mma<4>(a, ev_tile + li * IG_LD + lk, IgMask{need}, prod);
                }
                const int row = rb + li;
                if (row < rows_c) {
                    const double c5 = h5m[row];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (oinst[r] < 0) continue;
                        const size_t at = (size_t)oinst[r] * m0 + row;
                        double rhs = prod[r];
                        if (kc0) rhs += part[at];
                        if (!last) { part[at] = rhs; continue; }
                        const double res = hv[at] - rhs - c5;
                        if (res > best[r] || brow_[r] < 0) { best[r] = res; brow_[r] = row; }
                    }
                }
            }
        }
        if (cols.per_col) ev_write(best, brow_, oinst, dead, li, (size_t)cols.ld_out, cols.col0 + c, vio, row_out);
    }
    if (!cols.per_col) ev_write(best, brow_, oinst, dead, li, 1, 0, vio, row_out);
}

// the same on the vector ALUs (MLD_DBG_GEMM_VALU): one workgroup per instance, its plan and then H_v v in LDS, a wave per row with the lanes along the
// inner dimension.  The full products, without the causal skip: agreement with k_evaluate also checks the skip.
__global__ void __launch_bounds__(256) k_evaluate_valu(int m0, int n, int nx, int nW, const double *Hv, const double *Hx, const double *Hw, const double *H5,
                                                       const int *model_idx, const double *v, const int *status, const double *obj, int do_v, EvCols cols,
                                                       double *hv, double *vio, int *row_out)
{
    extern __shared__ double ev_in[];      // n doubles of v, then m0 of H_v v
    __shared__ double wbest[4]; __shared__ int wrow[4];
    const int b = blockIdx.x, mdl = model_idx ? model_idx[b] : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    double *hvl = ev_in + n;
    const double *h5m = H5 + (size_t)mdl * m0;
    if (do_v) {
        for (int k = threadIdx.x; k < n; k += blockDim.x) ev_in[k] = v[(size_t)b * n + k];
        __syncthreads();
        for (int row = wave; row < m0; row += nwv) {
            double s = 0.0;
            if (Hv) { const double *pm = Hv + ((size_t)mdl * m0 + row) * n; for (int k = lane; k < n; k += 64) s += pm[k] * ev_in[k]; }
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
            if (lane == 0) { hvl[row] = s; hv[(size_t)b * m0 + row] = s; }
        }
    } else
        for (int row = threadIdx.x; row < m0; row += blockDim.x) hvl[row] = hv[(size_t)b * m0 + row];
    __syncthreads();
    const bool dead = status && !plan_usable(status, obj, b);
    const double ninf = -__builtin_huge_val();
    const int ncols = cols.std + cols.n_cols;
    double best = ninf; int brow = -1;      // (lane 0 of every wave)
    auto flush = [&](size_t at) {
        if (lane == 0) { wbest[wave] = best; wrow[wave] = brow; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double bb = ninf; int ww = -1;
            for (int q = 0; q < nwv; ++q) if (wrow[q] >= 0 && (ww < 0 || wbest[q] > bb || (wbest[q] == bb && wrow[q] < ww))) { bb = wbest[q]; ww = wrow[q]; }
            if (vio) vio[at] = dead ? __builtin_nan("") : bb;
            if (row_out) row_out[at] = dead ? -1 : ww;
        }
        __syncthreads();
    };
    for (int c = 0; c < ncols; ++c) {
        const bool own = cols.std && c == 0;
        const int j = c - cols.std;
        const int rows_c = own || !cols.rows ? m0 : min(cols.rows[j], m0);
        const double *xs = own || !cols.xc ? cols.x0 + (size_t)b * nx : cols.xc + ((size_t)b * cols.n_cols + j) * nx;
        const double *ws = own ? cols.omega + (size_t)b * nW : cols.omc + ((size_t)b * cols.n_cols + j) * nW;
        if (cols.per_col) { best = ninf; brow = -1; }
        for (int row = wave; row < rows_c; row += nwv) {
            double s = 0.0;
            if (Hx) { const double *pm = Hx + ((size_t)mdl * m0 + row) * nx; for (int k = lane; k < nx; k += 64) s += pm[k] * xs[k]; }
            if (Hw) { const double *pm = Hw + ((size_t)mdl * m0 + row) * nW; for (int k = lane; k < nW; k += 64) s += pm[k] * ws[k]; }
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
            const double res = hvl[row] - s - h5m[row];
            if (lane == 0 && (res > best || brow < 0)) { best = res; brow = row; }
        }
        if (cols.per_col) flush((size_t)b * cols.ld_out + cols.col0 + c);
    }
    if (!cols.per_col) flush((size_t)b);
}

// int_vio[b] = max over the binaries |v_j - rint(v_j)|, bound_vio[b] = the largest violation of the declared bounds (mu >= 0, binaries in [0, 1],
// everything else free; controllers/components/variables.py:189-243).  The kinds follow from a variable's position inside its step
// [u (the last nu_l binary) | delta (binary) | z | mu (>= 0, the last nmu_l binary)].  A wave per instance; exact (elementwise fp64 and a maximum).
__global__ void __launch_bounds__(256) k_eval_point(int batch, int n, int nv, int nu, int nu_l, int nd, int nz, int nmu, int nmu_l, const double *v,
                                                   const int *status, const double *obj, double *int_vio, double *bound_vio)
{
    const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= batch) return;
    const int omu = nu + nd + nz;
    double iv = 0.0, bv = 0.0;
    for (int k = lane; k < n; k += 64) {
        const int pos = k % nv;
        const double x = v[(size_t)b * n + k];
        const bool is_mu = pos >= omu;
        const bool bin = (pos >= nu - nu_l && pos < nu + nd) || pos >= omu + nmu - nmu_l;
        if (bin) { iv = fmax(iv, fabs(x - rint(x))); bv = fmax(bv, fmax(0.0 - x, x - 1.0)); }
        else if (is_mu) bv = fmax(bv, 0.0 - x);
    }
    for (int o = 32; o > 0; o >>= 1) { iv = fmax(iv, __shfl_down(iv, o, 64)); bv = fmax(bv, __shfl_down(bv, o, 64)); }
    if (lane == 0) {
        const bool dead = status && !plan_usable(status, obj, b);
        if (int_vio) int_vio[b] = dead ? __builtin_nan("") : iv;
        if (bound_vio) bound_vio[b] = dead ? __builtin_nan("") : bv;
    }
}

// obj[b] = 1/2 v'Pv + q'v + cx'x0 + cw'omega + c0 + rconst[b]: the value k_solve reports (problem.inc: r_const) for the plan v at the current inputs.
// q: the per-instance linear term (batch x n, UNSCALED: k_qinst / k_inst_cost run with unit column scales) or null = the model's q0; P null = linear cost.
// One workgroup per instance, v in LDS, a wave per row of P.
__global__ void __launch_bounds__(256) k_eval_obj(int n, int nx, int nW, const double *q0, const double *qi, const double *P, const double *cx, const double *cw,
                                                 const double *c0, const double *rconst, const int *model_idx, const double *v, const double *x0,
                                                 const double *omega, const int *status, const double *obj, double *out)
{
    extern __shared__ double ev_v[];
    __shared__ double part[4];
    const int b = blockIdx.x, mdl = model_idx ? model_idx[b] : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    for (int k = threadIdx.x; k < n; k += blockDim.x) ev_v[k] = v[(size_t)b * n + k];
    __syncthreads();
    double s = 0.0;
    if (P) {
        const double *Pm = P + (size_t)mdl * n * n;
        for (int i = wave; i < n; i += nwv) {
            double a = 0.0;
            for (int k = lane; k < n; k += 64) a += Pm[(size_t)i * n + k] * ev_v[k];
            s += 0.5 * a * ev_v[i];
        }
    }
    const double *q = qi ? qi + (size_t)b * n : q0 + (size_t)mdl * n;
    for (int k = threadIdx.x; k < n; k += blockDim.x) s += q[k] * ev_v[k];
    if (cx) for (int k = threadIdx.x; k < nx; k += blockDim.x) s += cx[(size_t)mdl * nx + k] * x0[(size_t)b * nx + k];
    if (cw) for (int k = threadIdx.x; k < nW; k += blockDim.x) s += cw[(size_t)mdl * nW + k] * omega[(size_t)b * nW + k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < nwv; ++w) t += part[w];
        t += (c0 ? c0[mdl] : 0.0) + (rconst ? rconst[b] : 0.0);
        out[b] = (status && !plan_usable(status, obj, b)) ? __builtin_nan("") : t;
    }
}
