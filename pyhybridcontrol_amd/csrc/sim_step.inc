// One plant step of the resident batch with the WHOLE step-0 slice given -- the reference's MldModel.lsim_k(x_k, v_k=[u; delta; z; mu], omega_k)
// (models/mld_model.py:647-699 with :666-676: no auxiliary resolution), called by ControllerBase.sim_step_k (controllers/controller_base.py:229-253) and
// logged into MldSimLog (:58-146):
//     x_k1 = b5 + A x + [B1 B2 B3 0] v + B4 omega                                                    (:690)
//     y    = d5 + C x + [D1 D2 D3 0] v + D4 omega                                                    (:691)
//     r    = E x + [F1 F2 F3] (u, delta, z) + F4 omega + G y - f5 ,  cons = r <= 1e-6                (:692-694: the Psi mu term is zeroed)
//     cons_vio = max_i r_i ,  cons_row = the lowest row that attains it                              (-inf, -1 without rows; a NaN residual wins: a flag that
//                                                                                                      cannot be computed must not read as "consistent")
// omega is the forecast's step 0 or, under MLD_SIM_ACTUAL, one element run of the profile library (the window rule of profiles.inc with one step).
// Everything is fp64 on the ORIGINAL matrices of mld_model::d_pack, also on an MLD_F32 handle.  The sums and the rules of the maximum are plant_step.inc's,
// the one definition k_advance and k_rollout call too, so an advance through this kernel leaves the bits k_advance leaves.
//
// Mapping: one 64-lane wave per instance, four per workgroup, workgroups stride over the batch.  A step is a handful of short dot products per instance
// (cfg4: 7 + 1 + 20 rows over 38 terms): the model's matrices stay in cache, the traffic is the instance's own [x; v0; omega] and its record.  The wave
// stages [x; v0; omega] in LDS once (reads are broadcasts), lanes take output rows i = lane, lane + 64, ...: first the nx + ny rows, then -- y parked in
// LDS -- the nc rows; the maximum residual is reduced with __shfl_xor, ties to the lower row.  Every store of a record is lane-contiguous.  Shapes whose
// staging does not fit the workgroup's LDS (SS_LDS_MAX) read x, v0, omega and y from global memory instead (`lds` = 0; the realised omega and y then go
// through scratch the host supplies): the same sums in the same order, so the two paths agree bit for bit.  No dimension is a compile-time constant.
#pragma once

#define SS_WAVES 4
#define SS_LDS_MAX ((size_t)48 << 10)      /* dynamic LDS of one workgroup the staging may use (the default limit of a launch is 64 KB) */

struct SimStepArgs {
    int batch, nx, nv, nmu, nw, ny, nc, N, lds;
    const double *pack; size_t pack_len;
    PackOff off;                                /* offsets inside a model's packed block (mld_model_create) */
    const int *model_idx;
    const double *x0, *omega;                   /* current inputs: (batch, nx), (batch, N nw) */
    const double *v; size_t v_stride;           /* step-0 slices are the first nv entries of a row */
    const int *status; const double *obj;       /* resident plan: instances without a usable plan are masked; nullptr = the caller's v0, no masking */
    const unsigned char *mask;                  /* nullptr: the rule above; else the usable flag per instance itself (k_aux_merge), status / obj only go into the record */
    const double *lbnd; const int *nodes;       /* copied into the record (nullptr: NaN / 0) */
    const long long *act_start; const PfChan *chan; int n_groups, step; const double *lib;      /* act_start == nullptr: the forecast's step 0 */
    double *x0_new, *omega_new;                 /* MLD_SIM_ADVANCE: the spare input buffers (nullptr otherwise) */
    /* outputs / record fields, any nullptr: (batch, width) each */
    double *x_k1, *y, *vio; unsigned char *cons; int *row;
    double *rec_x, *rec_v, *rec_om, *rec_obj, *rec_lb; int *rec_status, *rec_nodes;
    double *w_tmp, *y_tmp;                      /* lds == 0: scratch of the realised omega (batch, nw) and of y (batch, ny) between the row passes */
    int *n_skipped;
};

__global__ void __launch_bounds__(64 * SS_WAVES) k_sim_step(const SimStepArgs a)
{
    extern __shared__ double ss_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nx = a.nx, nv = a.nv, nw = a.nw, ny = a.ny, nc = a.nc, nf = a.nv - a.nmu;
    const size_t nW = (size_t)a.N * nw;
    const double qnan = __builtin_nan("");
    double *const xs = ss_lds + (size_t)wave * (nx + nv + nw + ny), *const vs = xs + nx, *const ws = vs + nv, *const ys = ws + nw;
    for (long long base = (long long)blockIdx.x * SS_WAVES; base < a.batch; base += (long long)gridDim.x * SS_WAVES) {      /* uniform over the workgroup */
        const long long b = base + wave;
        const bool live = b < a.batch;
        const bool usable = live && (a.mask ? a.mask[b] != 0 : (!a.status || plan_usable(a.status, a.obj, (int)b)));
        const double *xg = a.x0 + (live ? b : 0) * nx, *vg = a.v + (live ? b : 0) * a.v_stride, *fg = a.omega + (live ? b : 0) * nW;
        const double *pk = a.pack + (size_t)(live && a.model_idx ? a.model_idx[b] : 0) * a.pack_len;
        /* ---- inputs: staged in LDS, and copied into the record ------------------------------------------------------------------------------- */
        if (live) {
            for (int j = lane; j < nx; j += 64) { const double t = xg[j]; if (a.lds) xs[j] = t; if (a.rec_x) a.rec_x[b * nx + j] = t; }
            for (int j = lane; j < nv; j += 64) { const double t = vg[j]; if (a.lds) vs[j] = t; if (a.rec_v) a.rec_v[b * nv + j] = usable ? t : qnan; }
            for (int j = lane; j < nw; j += 64) {
                double t;
                if (a.act_start) { const PfChan ch = a.chan[j]; t = a.lib[a.act_start[b * a.n_groups + ch.group] + (long long)a.step * ch.width + ch.off]; }
                else t = fg[j];
                if (a.lds) ws[j] = t; else if (a.act_start) a.w_tmp[b * nw + j] = t;
                if (a.rec_om) a.rec_om[b * nw + j] = t;
            }
            if (lane == 0) {
                if (!usable && a.n_skipped) atomicAdd(a.n_skipped, 1);
                if (a.rec_obj) a.rec_obj[b] = a.obj ? a.obj[b] : qnan;
                if (a.rec_lb) a.rec_lb[b] = a.lbnd ? a.lbnd[b] : qnan;
                if (a.rec_status) a.rec_status[b] = a.status ? a.status[b] : -1;
                if (a.rec_nodes) a.rec_nodes[b] = a.nodes ? a.nodes[b] : 0;
            }
        }
        __syncthreads();
        const double *xr = a.lds ? xs : xg, *vr = a.lds ? vs : vg;
        const double *wr = a.lds ? ws : (a.act_start ? a.w_tmp + (live ? b : 0) * nw : fg);
        /* ---- state and output rows --------------------------------------------------------------------------------------------------------- */
        if (live) {
            for (int i = lane; i < nx; i += 64) {
                const double s = plant_row(i, pk + a.off.b5, pk + a.off.A, pk + a.off.Bv, pk + a.off.B4, nx, nv, nw, xr, vr, wr);
                if (a.x_k1) a.x_k1[b * nx + i] = usable ? s : qnan;
                if (a.x0_new) a.x0_new[b * nx + i] = usable ? s : xg[i];      /* no plan: the plant of this instance is not advanced */
            }
            for (int i = lane; i < ny; i += 64) {
                const double s = plant_row(i, pk + a.off.d5, pk + a.off.C, pk + a.off.Dv, pk + a.off.D4, nx, nv, nw, xr, vr, wr);
                if (a.lds) ys[i] = s; else a.y_tmp[b * ny + i] = s;
                if (a.y) a.y[b * ny + i] = usable ? s : qnan;
            }
            if (a.omega_new)      /* the forecast moves on by one step, the first step re-enters at the end (as k_advance) */
                for (size_t e = lane; e < nW; e += 64) {
                    const size_t k = e / nw, c = e - k * nw;
                    a.omega_new[b * nW + e] = usable ? fg[((k + 1) % a.N) * nw + c] : fg[e];
                }
        }
        __syncthreads();
        /* ---- constraint rows ------------------------------------------------------------------------------------------------------------- */
        const double *yr = a.lds ? ys : a.y_tmp + (live ? b : 0) * ny;
        double best = -INFINITY; int brow = -1;
        if (live) {
            for (int i = lane; i < nc; i += 64) {
                const double s = plant_residual(i, pk + a.off.E, pk + a.off.Fv, pk + a.off.F4, pk + a.off.G, pk + a.off.f5, nx, nv, nf, nw, ny, xr, vr, wr, yr);
                if (a.cons) a.cons[b * nc + i] = (usable && s <= 1.0e-6) ? 1 : 0;
                plant_worst(s, i, best, brow);
            }
        }
        for (int off = 32; off; off >>= 1) plant_worst_merge(__shfl_xor(best, off), __shfl_xor(brow, off), best, brow);
        if (live && lane == 0) {
            if (a.vio) a.vio[b] = usable ? best : qnan;
            if (a.row) a.row[b] = usable ? brow : -1;
        }
        __syncthreads();      /* the constraint rows have read the staging before the next instance overwrites it */
    }
}
