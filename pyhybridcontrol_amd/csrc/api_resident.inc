// Services on the resident batch between solves: disturbance profiles, per-instance cost, predicted trajectories, solution quality, receding
// horizon, plant step (with the planned auxiliaries or with re-derived ones) and simulation log.
extern "C" {

/* ---- resident disturbance profiles ----------------------------------------------------------------------------------------------------------------
 * The reference cuts every disturbance window out of a series it holds once (get_omega_tilde_k_hat / _act, modelling/micro_grid_agents.py:236-298;
 * get_omega_tilde_scenario, :206-232); here the series are a flat library in HBM and a window is a start offset (profiles.inc: k_profile_windows and the
 * window rule).  Every start is tested on the host before anything is queued: no kernel is launched with an offset that has not passed. */
int mld_upload_profiles(mld_problem_t *p, int64_t lib_len, const double *lib, int n_groups, const int32_t *group_width)
{
    if (int rc = entry_guard(p, "mld_upload_profiles", true, nullptr)) return rc;
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
        p->pf_lib.reset(); p->pf_chan.reset(); reset_profile_starts(p);
        p->pf_len = 0; p->pf_groups = 0; p->pf_width.clear();
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
    if (int rc = queue_and_wait(sq, queue)) return rc;
    p->pf_lib = std::move(d_lib); p->pf_chan = std::move(d_chan);
    p->pf_len = lib_len; p->pf_groups = (int)width.size(); p->pf_width = width;
    reset_profile_starts(p);      /* they pointed into the library that is gone */
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
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    int rc;
    if ((rc = profile_ready(p, who, step))) return rc;
    const int batch = p->batch, G = p->pf_groups;
    std::vector<long long> gmax;
    if (start) { if ((rc = profile_check_starts(p, who, PF_WINDOW, start, batch, 1, step, p->N, gmax))) return rc; }
    else {
        if (p->pf_forecast.batch != batch) { mld_set_error("%s: start == NULL, but no starts of this batch are resident (pass them once)", who); return MLD_ERR_INVALID; }
        if ((rc = profile_check_resident(p, who, PF_WINDOW, p->pf_forecast.gmax, step, p->N))) return rc;
    }
    DevBuf<long long> d_start;
    if (start) HIP_TRY(d_start.alloc((size_t)batch * G));
    const hipStream_t sq = p->stream;
    /* the new forecast is gathered into the spare input buffer and swapped in once the stream has finished: a call that fails changes nothing */
    auto queue = [&]() -> int {
        if (start) HIP_TRY(hipMemcpyAsync(d_start, start, sizeof(long long) * (size_t)batch * G, hipMemcpyHostToDevice, sq));
        launch_profile_windows(p, sq, batch, 1, 1, 0, start ? d_start.get() : p->pf_forecast.d.get(), step, p->bat.omegab.get());
        HIP_TRY(hipGetLastError());
        return MLD_OK;
    };
    if ((rc = queue_and_wait(sq, queue))) return rc;
    std::swap(p->bat.omega, p->bat.omegab);
    if (start) set_starts(p->pf_forecast, std::move(d_start), batch, 1, gmax);
    forecast_replaced(p);
    return MLD_OK;
}

int mld_constraint_blocks_from_profiles(mld_problem_t *p, int n_cols, const int64_t *start, int step, const int32_t *col_rows, const double *x_cols)
{
    static const char who[] = "mld_constraint_blocks_from_profiles";
    if (int rc = entry_guard(p, who, true, "upload the batch first")) return rc;
    if (n_cols < 0) { mld_set_error("%s: n_cols = %d", who, n_cols); return MLD_ERR_INVALID; }
    if (n_cols == 0) { p->n_xcols = 0; return MLD_OK; }
    int rc;
    if ((rc = profile_ready(p, who, step))) return rc;
    const int batch = p->batch, G = p->pf_groups;
    if ((long long)batch * n_cols > INT_MAX) { mld_set_error("%s: batch x n_cols = %lld windows (at most %d)", who, (long long)batch * n_cols, INT_MAX); return MLD_ERR_INVALID; }
    if ((rc = check_col_rows(p, who, n_cols, col_rows))) return rc;
    std::vector<long long> gmax;
    if (start) { if ((rc = profile_check_starts(p, who, PF_WINDOW, start, batch, n_cols, step, p->N, gmax))) return rc; }
    else {
        if (p->pf_columns.batch != batch) { mld_set_error("%s: start == NULL, but no column starts of this batch are resident (pass them once)", who); return MLD_ERR_INVALID; }
        if (p->pf_columns.cols != n_cols) { mld_set_error("%s: start == NULL with n_cols = %d, but the resident starts are those of %d columns", who, n_cols, p->pf_columns.cols); return MLD_ERR_INVALID; }
        if ((rc = profile_check_resident(p, who, PF_WINDOW, p->pf_columns.gmax, step, p->N))) return rc;
    }
    DevBuf<long long> d_start;
    if (start) HIP_TRY(d_start.alloc((size_t)batch * n_cols * G));
    const bool with_x = x_cols && p->nx;
    if ((rc = stage_xcols(p, n_cols, col_rows != nullptr, with_x))) return rc;
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int {
        if (start) HIP_TRY(hipMemcpyAsync(d_start, start, sizeof(long long) * (size_t)batch * n_cols * G, hipMemcpyHostToDevice, sq));
        if (col_rows) HIP_TRY(hipMemcpyAsync(p->bat.xrows, col_rows, sizeof(int) * n_cols, hipMemcpyHostToDevice, sq));
        if (with_x) HIP_TRY(hipMemcpyAsync(p->bat.xcols_x, x_cols, sizeof(double) * (size_t)batch * n_cols * p->nx, hipMemcpyHostToDevice, sq));
        launch_profile_windows(p, sq, batch * n_cols, n_cols, n_cols, 0, start ? d_start.get() : p->pf_columns.d.get(), step, p->bat.xcols.get());
        HIP_TRY(hipGetLastError());
        return MLD_OK;
    };
    if ((rc = queue_and_wait(sq, queue))) return rc;
    if (start) set_starts(p->pf_columns, std::move(d_start), batch, n_cols, gmax);
    p->n_xcols = n_cols;
    return MLD_OK;
}

int mld_download_constraint_blocks(mld_problem_t *p, int32_t *n_cols_out, double *omega_cols, int32_t *col_rows, double *x_cols)
{
    if (int rc = entry_guard(p, "mld_download_constraint_blocks", false, "nothing uploaded")) return rc;
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
/* The tail the two routes to a per-instance cost share (the caller's weights: mld_upload_instance_cost; weights built on the device from price windows:
 * mld_instance_cost_from_prices).  inst_cost_ld: the row length of the new cost.  queue_inst_pullback: with the weights on [x_tilde | y_tilde] in d_w
 * (batch, NX + NY) and lin_v in the first n columns of ic, the GEMM that completes ic.  adopt_inst_cost: the new cost becomes the resident one. */
static int inst_cost_ld(const mld_problem *p, bool pull) { return pull ? p->n + p->nx + p->nW + 1 : p->n; }      /* weights on v only: no GEMM, cx / cw / c0 are zero and not stored */

static int queue_inst_pullback(mld_problem *p, hipStream_t sq, const double *d_w, double *ic)
{
    const int NX = p->N * p->model->dims.nx, NY = p->N * p->model->dims.ny, K = NX + NY;
    const PbMaps mp = pullback_maps(p);
    if (p->opts.reserved & MLD_DBG_GEMM_VALU)
        hipLaunchKernelGGL(k_inst_pullback_valu, dim3(p->batch), dim3(256), sizeof(double) * K, sq, NX, NY, p->n, p->nx, p->nW, mp, p->has_midx ? p->bat.model_idx.get() : nullptr, d_w, ic);
    else
        LAUNCH_INST_GEMM(k_inst_pullback, p->opts.flags & MLD_F32, p->n_groups, 0, sq, NX, NY, p->n, p->nx, p->nW, mp, p->bat.groups.get(), p->bat.perm.get(), d_w, ic);
    HIP_TRY(hipGetLastError());
    return MLD_OK;
}

static void adopt_inst_cost(mld_problem *p, DevBuf<double> &&ic, int ld) { p->bat.icost = std::move(ic); p->ic_ld = ld; }

int mld_upload_instance_cost(mld_problem_t *p, const double *lin_v, const double *lin_x, const double *lin_y)
{
    if (int rc = entry_guard(p, "mld_upload_instance_cost", true, "upload a batch first (the cost belongs to its instances)")) return rc;
    const int n = p->n, batch = p->batch;
    const int NX = p->N * p->model->dims.nx, NY = p->N * p->model->dims.ny;
    if (lin_x && NX == 0) { mld_set_error("mld_upload_instance_cost: lin_x given but the model has no state (nx = 0)"); return MLD_ERR_INVALID; }
    if (lin_y && NY == 0) { mld_set_error("mld_upload_instance_cost: lin_y given but the model has no output (ny = 0)"); return MLD_ERR_INVALID; }
    if (!lin_v && !lin_x && !lin_y) { p->bat.icost.reset(); p->bat.qs_inst_t.reset(); p->ic_ld = 0; return MLD_OK; }
    const hipStream_t sq = p->stream;
    const bool pull = lin_x || lin_y;
    const int ld = inst_cost_ld(p, pull);
    DevBuf<double> ic, d_w;
    HIP_TRY(ic.alloc((size_t)batch * std::max(1, ld)));
    /* everything queued on the stream and waited for on every path (queue_and_wait): the caller's arrays and the temporaries may go when this returns */
    auto queue = [&]() -> int {
    if (!lin_v || pull) HIP_TRY(hipMemsetAsync(ic, 0, sizeof(double) * (size_t)batch * std::max(1, ld), sq));
    if (lin_v && n && !pull) HIP_TRY(hipMemcpyAsync(ic, lin_v, sizeof(double) * (size_t)batch * n, hipMemcpyHostToDevice, sq));      /* rows are contiguous: one plain copy */
    else if (lin_v && n) HIP_TRY(hipMemcpy2DAsync(ic, sizeof(double) * ld, lin_v, sizeof(double) * n, sizeof(double) * n, batch, hipMemcpyHostToDevice, sq));
    if (pull) {
        const int K = NX + NY;
        HIP_TRY(d_w.alloc((size_t)batch * K));
        if (!lin_x || !lin_y) HIP_TRY(hipMemsetAsync(d_w, 0, sizeof(double) * (size_t)batch * K, sq));
        if (lin_x) HIP_TRY(hipMemcpy2DAsync(d_w, sizeof(double) * K, lin_x, sizeof(double) * NX, sizeof(double) * NX, batch, hipMemcpyHostToDevice, sq));
        if (lin_y) HIP_TRY(hipMemcpy2DAsync(d_w.get() + NX, sizeof(double) * K, lin_y, sizeof(double) * NY, sizeof(double) * NY, batch, hipMemcpyHostToDevice, sq));
        if (int rc = queue_inst_pullback(p, sq, d_w.get(), ic.get())) return rc;
    }
    return MLD_OK;
    };
    if (int rc = queue_and_wait(sq, queue)) return rc;
    adopt_inst_cost(p, std::move(ic), ld);
    return MLD_OK;
}

int mld_download_instance_cost(mld_problem_t *p, double *q_out, double *const_out)
{
    if (int rc = entry_guard(p, "mld_download_instance_cost", false, "nothing uploaded")) return rc;
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
    if (int rc = entry_guard(p, "mld_predict_batch", true, "no batch resident (mld_upload_batch)")) return rc;
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
    /* everything queued on the stream and waited for on every path (queue_and_wait): the caller's arrays and the temporaries may go when this returns */
    auto queue = [&]() -> int {
        if (v && n) HIP_TRY(hipMemcpyAsync(d_v, v, sizeof(double) * (size_t)batch * n, hipMemcpyHostToDevice, sq));
        const double *pv = v ? d_v.get() : p->bat.v.get();      /* (the resident solution: rows < batch are the instances', hand-off items come after them) */
        const int *st = v ? nullptr : p->bat.status.get();
        const double *ob = v ? nullptr : p->bat.obj.get();
        const PbMaps mp = pullback_maps(p);
        const int r_begin = x_out ? 0 : NX, r_end = y_out ? NX + NY : NX;      /* rows of the stacked maps that are asked for */
        if (p->opts.reserved & MLD_DBG_GEMM_VALU)
            hipLaunchKernelGGL(k_trajectory_valu, dim3(batch), dim3(256), sizeof(double) * (n + nx + nW + 1), sq, NX, NY, n, nx, nW, mp,
                               p->has_midx ? p->bat.model_idx.get() : nullptr, pv, p->bat.x0.get(), p->bat.omega.get(), st, ob, r_begin, r_end, d_x.get(), d_y.get());
        else
            LAUNCH_INST_GEMM(k_trajectory, p->opts.flags & MLD_F32, p->n_groups, 0, sq, N, d.nx, d.ny, p->nv, d.nomega, mp, p->bat.groups.get(), p->bat.perm.get(),
                             pv, p->bat.x0.get(), p->bat.omega.get(), st, ob, r_begin, r_end, d_x.get(), d_y.get());
        HIP_TRY(hipGetLastError());
        if (x_out) HIP_TRY(hipMemcpyAsync(x_out, d_x, sizeof(double) * (size_t)batch * NX, hipMemcpyDeviceToHost, sq));
        if (y_out) HIP_TRY(hipMemcpyAsync(y_out, d_y, sizeof(double) * (size_t)batch * NY, hipMemcpyDeviceToHost, sq));
        return MLD_OK;
    };
    return queue_and_wait(sq, queue);
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
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const mld_dims &d = p->model->dims;
    const int n = p->n, nx = p->nx, nW = p->nW, batch = p->batch, m0 = p->m0, M = p->n_models;
    if (n_cols < 0) { mld_set_error("%s: n_cols = %d", who, n_cols); return MLD_ERR_INVALID; }
    if (!from_profiles && n_cols > 0 && nW && !omega_cols) { mld_set_error("%s: n_cols = %d without omega_cols (nomega > 0)", who, n_cols); return MLD_ERR_INVALID; }
    if (from_profiles && n_cols < 1) { mld_set_error("%s: n_cols = %d (the profile columns of a call: at least one)", who, n_cols); return MLD_ERR_INVALID; }
    if (from_profiles && !start) { mld_set_error("%s: start == NULL (the resident column starts belong to the problem's blocks and are not used here)", who); return MLD_ERR_INVALID; }
    if (x_cols && nx == 0) { mld_set_error("%s: x_cols given but the model has no state (nx = 0)", who); return MLD_ERR_INVALID; }
    if (int rc = check_col_rows(p, who, n_cols, col_rows)) return rc;
    if (!v && !p->solved) { mld_set_error("%s: the resident batch has not been solved since its upload / selection (there is no plan to evaluate; pass v)", who); return MLD_ERR_INVALID; }
    if (!v && p->advanced) { mld_set_error("%s: mld_advance_batch has moved the inputs on -- the resident plan belongs to inputs that are gone (solve again, or pass v)", who); return MLD_ERR_INVALID; }
    int rc;
    if (from_profiles) {      /* every start against the window rule, before anything is queued */
        std::vector<long long> gmax;
        if ((rc = profile_ready(p, who, step))) return rc;
        if ((long long)batch * n_cols > INT_MAX) { mld_set_error("%s: batch x n_cols = %lld windows (at most %d)", who, (long long)batch * n_cols, INT_MAX); return MLD_ERR_INVALID; }
        if ((rc = profile_check_starts(p, who, PF_WINDOW, start, batch, n_cols, step, p->N, gmax))) return rc;
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
        if (!valu && nx + nW > IG_KC) HIP_TRY(d_part.alloc((size_t)batch * std::max(1, m0)));
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
    /* everything queued on the stream and waited for on every path (queue_and_wait): the caller's arrays and the temporaries may go when this returns */
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
            /* the per-instance q and constant at the current inputs as the solve path computes them, with unit column scales and into buffers of this
             * call (the solve path's qs_inst / rconst are not touched) */
            if (inst_q) {
                const size_t one = (size_t)std::max(1, n) * M;
                hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)((one + 255) / 256)), dim3(256), 0, sq, one, 1.0, d_one.get());
                if (int rc = launch_instance_cost(p, d_one.get(), d_qi.get(), d_rc.get(), nullptr, nullptr)) return rc;
            }
            hipLaunchKernelGGL(k_eval_obj, dim3(batch), dim3(256), sizeof(double) * std::max(1, n), sq, n, nx, nW, p->d_q0.get(), inst_q ? d_qi.get() : nullptr,
                               p->has_quad ? p->d_P.get() : nullptr, nx ? p->d_cx.get() : nullptr, nW ? p->d_cw.get() : nullptr, p->d_c0.get(),
                               inst_q ? d_rc.get() : nullptr, midx, pv, p->bat.x0.get(), p->bat.omega.get(), st, ob, d_obj.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(obj_out, d_obj, sizeof(double) * batch, hipMemcpyDeviceToHost, sq));
        }
        return MLD_OK;
    };
    return queue_and_wait(sq, queue);
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

int mld_advance_batch2(mld_problem_t *p, int32_t *n_skipped_out)
{
    if (int rc = entry_guard(p, "mld_advance_batch", false, "nothing uploaded / solved")) return rc;
    if (!p->solved) { mld_set_error("mld_advance_batch: the resident batch has not been solved since its upload / selection (there is no plan to apply)"); return MLD_ERR_INVALID; }
    if (p->advanced) { mld_set_error("mld_advance_batch: the last solve's plan has already been applied -- solve the advanced batch first (a second advance would apply the same step-0 inputs to a state that has moved on)"); return MLD_ERR_INVALID; }
    mld_model *m = p->model;
    const mld_dims &d = m->dims;
    if (!m->d_pack) { mld_set_error("mld_advance_batch: model without matrices"); return MLD_ERR_INVALID; }
    if (m->tv_N > 0) { mld_set_error("mld_advance_batch: time-varying models (mld_model_create_tv) are not advanced on the device -- the step models would have to shift with the horizon"); return MLD_ERR_INVALID; }
    const size_t bx = ((size_t)p->batch * std::max(1, p->nx) + 255) / 256, bw = ((size_t)p->batch * std::max(1, p->nW) + 255) / 256;
    const int grid = (int)std::max<size_t>(bx, std::min<size_t>(bw, (size_t)1 << 20));   /* the state part is one thread per element, the shift strides */
    HIP_TRY(hipMemsetAsync(p->bat.skipped, 0, sizeof(int), p->stream));
    hipLaunchKernelGGL(k_advance, dim3(grid), dim3(256), 0, p->stream, p->batch, p->nx, p->nv, d.nomega, p->N,
                       m->d_pack, m->pack_len, m->pack_off,
                       p->has_midx ? p->bat.model_idx : nullptr, p->bat.x0, p->bat.omega, p->bat.v, (size_t)p->n, p->bat.x0b, p->bat.omegab,
                       p->bat.status, p->bat.obj, p->bat.skipped);
    HIP_TRY(hipGetLastError());
    int skipped = 0;
    HIP_TRY(hipMemcpyAsync(&skipped, p->bat.skipped, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    std::swap(p->bat.x0, p->bat.x0b); std::swap(p->bat.omega, p->bat.omegab);
    inputs_advanced_by_plan(p);
    if (n_skipped_out) *n_skipped_out = skipped;
    return MLD_OK;
}

int mld_advance_batch(mld_problem_t *p) { return mld_advance_batch2(p, nullptr); }

/* ---- plant step and simulation log of the resident batch -------------------------------------------------------------------------------------------
 * One step of the reference's closed loop after the solve: ControllerBase.sim_step_k -> MldModel.lsim_k -> MldSimLog (controllers/controller_base.py:
 * 229-253, models/mld_model.py:647-699, controller_base.py:58-146), with the whole step-0 slice v0 = [u; delta; z; mu] given (lsim_k's v_k=, no
 * auxiliary resolution) -- the resident plan's or the caller's -- under the forecast's step 0 or the REALISED disturbance out of the profile library.
 * Kernel: sim_step.inc.  Everything is tested on the host before anything is queued, the new inputs are built in the spare buffers and swapped in by
 * the host, the starts of the realised series in a buffer of their own: a call that is refused changes nothing. */
int mld_sim_log_begin(mld_problem_t *p, int capacity)
{
    static const char who[] = "mld_sim_log_begin";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch): the log belongs to a batch")) return rc;
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

/* The host-side tests the two step entry points share, before anything is queued.  own: the caller brings the inputs (`arg`: v0 / u0), so no plan is needed.
 * gmax: per group the largest start of act_start, for set_starts once the step has been taken. */
static int sim_step_check(mld_problem_t *p, const char *who, bool own, const char *arg, const int64_t *act_start, int step, int flags, std::vector<long long> &gmax)
{
    mld_model *m = p->model;
    const int batch = p->batch, nw = m->dims.nomega;
    if (flags & ~(MLD_SIM_ADVANCE | MLD_SIM_ACTUAL | MLD_SIM_LOG)) { mld_set_error("%s: unknown flag bits 0x%x (MLD_SIM_ADVANCE | MLD_SIM_ACTUAL | MLD_SIM_LOG)", who, flags); return MLD_ERR_INVALID; }
    const bool actual = flags & MLD_SIM_ACTUAL, log = flags & MLD_SIM_LOG;
    if (step < 0 || step == INT_MAX) { mld_set_error("%s: step = %d (must be >= 0)", who, step); return MLD_ERR_INVALID; }
    if (m->tv_N > 0) { mld_set_error("%s: time-varying models (mld_model_create_tv) are not stepped on the device -- the step models would have to shift with the horizon (as mld_advance_batch)", who); return MLD_ERR_INVALID; }
    if (!m->d_pack) { mld_set_error("%s: model without matrices", who); return MLD_ERR_INVALID; }
    if (!own && !p->solved) { mld_set_error("%s: the resident batch has not been solved since its upload / selection (there is no plan to apply; pass %s)", who, arg); return MLD_ERR_INVALID; }
    if (!own && p->advanced) { mld_set_error("%s: the last solve's plan has already been applied -- the resident plan belongs to inputs that are gone (solve again, or pass %s)", who, arg); return MLD_ERR_INVALID; }
    if (act_start && !actual) { mld_set_error("%s: act_start given without MLD_SIM_ACTUAL", who); return MLD_ERR_INVALID; }
    if (actual) {
        if (nw == 0) { mld_set_error("%s: MLD_SIM_ACTUAL, but the model has no disturbance (nomega = 0)", who); return MLD_ERR_INVALID; }
        if (!p->pf_len) { mld_set_error("%s: MLD_SIM_ACTUAL, but no profile library is resident (mld_upload_profiles)", who); return MLD_ERR_INVALID; }
        /* the window rule with ONE step: s >= 0 and s + (step + 1) * width_g <= lib_len */
        if (act_start) { if (int rc = profile_check_starts(p, who, PF_ELEMENT, act_start, batch, 1, step, 1, gmax)) return rc; }
        else {
            if (p->pf_actual.batch != batch) { mld_set_error("%s: act_start == NULL, but no actual starts of this batch are resident (pass them once)", who); return MLD_ERR_INVALID; }
            if (int rc = profile_check_resident(p, who, PF_ELEMENT, p->pf_actual.gmax, step, 1)) return rc;
        }
    }
    const mld_problem::SimLog &L = p->slog;
    if (log && !L.cap) { mld_set_error("%s: MLD_SIM_LOG, but no log has been begun for this batch (mld_sim_log_begin)", who); return MLD_ERR_INVALID; }
    if (log && L.count >= L.cap) { mld_set_error("%s: MLD_SIM_LOG, but the log is full (%d of %d records; mld_download_sim_log, then mld_sim_log_begin)", who, L.count, L.cap); return MLD_ERR_INVALID; }
    /* the stage cost armed (mld_sim_log_cost_begin): the record's price is lib[s + step * n_chan ..], one element run of the price library */
    if (log && L.cost) { if (int rc = check_resident(price_lib(p), who, PF_PRICE_ELEMENT, std::vector<long long>(1, L.cstart_max), step, 1)) return rc; }
    return MLD_OK;
}

/* Where a step's slices come from.  Neither pointer: the resident plan.  v0: the caller's (batch, nv) on the host.  d_v0: slices the call has built on the
 * device (mld_sim_step_resolve) with their usable flag d_mask and resolver statuses d_auxst; by_plan says that their u was the resident plan's, so the record
 * carries the plan's obj / lower_bound / status / nodes and an advance leaves the handle `advanced`; d_start: act_start is on the device already. */
struct SimStepSrc {
    const double *v0 = nullptr, *d_v0 = nullptr; const unsigned char *d_mask = nullptr; const int *d_auxst = nullptr; bool by_plan = false;
    const AuxStepArgs *merge = nullptr;      /* k_aux_merge fills d_v0, d_mask and d_auxst: queued in front of the step */
    DevBuf<long long> *d_start = nullptr;
    double *v0_out = nullptr; int32_t *aux_status_out = nullptr;
};

/* the step itself, after sim_step_check: k_sim_step on the slices of `src`, the outputs, and -- queued without an error -- the handle moved on */
static int sim_step_run(mld_problem_t *p, const SimStepSrc &src, const int64_t *act_start, const std::vector<long long> &gmax, int step, int flags,
                        double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out, int32_t *n_skipped_out)
{
    mld_model *m = p->model;
    const mld_dims &d = m->dims;
    const int batch = p->batch, nx = d.nx, nv = p->nv, nw = d.nomega, ny = d.ny, nc = d.nc;
    const bool advance = flags & MLD_SIM_ADVANCE, actual = flags & MLD_SIM_ACTUAL, log = flags & MLD_SIM_LOG;
    const double *v0 = src.v0;
    const bool resolved = src.d_v0 != nullptr, plan = !v0 && !resolved;
    mld_problem::SimLog &L = p->slog;
    SimStepArgs a{};
    a.batch = batch; a.nx = nx; a.nv = nv; a.nmu = d.nmu; a.nw = nw; a.ny = ny; a.nc = nc; a.N = p->N;
    const size_t stage = sizeof(double) * SS_WAVES * ((size_t)nx + nv + nw + ny);
    a.lds = stage <= SS_LDS_MAX && !(p->opts.reserved & MLD_DBG_SIM_NO_LDS);
    a.pack = m->d_pack; a.pack_len = m->pack_len; a.off = m->pack_off;
    a.model_idx = p->has_midx ? p->bat.model_idx.get() : nullptr;
    a.x0 = p->bat.x0; a.omega = p->bat.omega;
    const hipStream_t sq = p->stream;
    DevBuf<double> d_v, d_xk1, d_y, d_vio; DevBuf<unsigned char> d_cons; DevBuf<int> d_row; DevBuf<long long> d_own_start;
    const bool up_start = act_start && !src.d_start;      /* the starts still have to go to the device */
    DevBuf<long long> &d_start = src.d_start ? *src.d_start : d_own_start;
    if (v0) HIP_TRY(d_v.alloc((size_t)batch * std::max(1, nv)));
    if (up_start) HIP_TRY(d_start.alloc((size_t)batch * p->pf_groups));
    if (!a.lds && !p->bat.sim_tmp) HIP_TRY(p->bat.sim_tmp.alloc((size_t)p->in_cap * std::max(1, nw + ny)));      /* sized like the input buffers (any batch up to in_cap); free_batch releases it with them */
    if (!a.lds) { a.w_tmp = p->bat.sim_tmp; a.y_tmp = p->bat.sim_tmp.get() + (size_t)batch * nw; }
    if (v0) { a.v = d_v; a.v_stride = (size_t)nv; }
    else if (resolved) { a.v = src.d_v0; a.v_stride = (size_t)nv; a.mask = src.d_mask; }
    else { a.v = p->bat.v; a.v_stride = (size_t)p->n; }      /* the resident plans: rows < batch are the instances' (after the hand-off's device merge), hand-off items come after them */
    if (plan || (resolved && src.by_plan)) { a.status = p->bat.status; a.obj = p->bat.obj; a.lbnd = p->bat.lbnd; a.nodes = p->bat.nodes; }
    if (actual) { a.act_start = act_start ? d_start.get() : p->pf_actual.d.get(); a.chan = p->pf_chan; a.n_groups = p->pf_groups; a.step = step; a.lib = p->pf_lib; }
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
     * advance on a stream of the problem's own, because the other entry points copy on the legacy stream, which does not order against that one.  A
     * resolving step is host-synchronous throughout: its temporaries go when it returns */
    const bool wait = v0 || resolved || up_start || count_skipped || x_k1_out || y_out || cons_out || cons_vio_out || cons_row_out || (advance && p->own_stream);
    auto queue = [&]() -> int {
        if (v0 && nv) HIP_TRY(hipMemcpyAsync(d_v, v0, sizeof(double) * (size_t)batch * nv, hipMemcpyHostToDevice, sq));
        if (up_start) HIP_TRY(hipMemcpyAsync(d_start, act_start, sizeof(long long) * (size_t)batch * p->pf_groups, hipMemcpyHostToDevice, sq));
        if (count_skipped) HIP_TRY(hipMemsetAsync(p->bat.skipped, 0, sizeof(int), sq));
        if (src.merge) {
            hipLaunchKernelGGL(k_aux_merge, dim3(profile_grid((long long)batch * std::max(1, nv))), dim3(256), 0, sq, *src.merge);
            HIP_TRY(hipGetLastError());
        }
        const int grid = (int)std::min<long long>(((long long)batch + SS_WAVES - 1) / SS_WAVES, 8192);
        hipLaunchKernelGGL(k_sim_step, dim3(grid), dim3(64 * SS_WAVES), a.lds ? stage : 0, sq, a);
        HIP_TRY(hipGetLastError());
        if (log && L.cost) {      /* the stage cost armed: price and cost of the record just written, the running total (k_stage_cost, prices.inc) */
            StageCostArgs c{};
            c.batch = batch; c.n_chan = p->pr_chan; c.nv = nv; c.ny = ny; c.step = step; c.model_idx = a.model_idx;
            c.mask = a.mask; c.status = a.status; c.obj = a.obj;
            c.start = L.cstart; c.lib = p->pr_lib; c.w_v = p->sc_tab; c.w_y = p->sc_tab.get() + (size_t)p->n_models * p->pr_chan * nv;
            c.rec_v = a.rec_v; c.rec_y = a.y; c.rec_cost = L.cost.get() + slot; c.rec_price = L.price.get() + slot * p->pr_chan;
            c.total = L.total; c.steps = L.steps;
            hipLaunchKernelGGL(k_stage_cost, dim3(profile_grid(batch)), dim3(256), 0, sq, c);
            HIP_TRY(hipGetLastError());
        }
        if (resolved && log) HIP_TRY(hipMemcpyAsync(L.aux.get() + slot, src.d_auxst, sizeof(int) * batch, hipMemcpyDeviceToDevice, sq));
        if (x_k1_out && nx) HIP_TRY(hipMemcpyAsync(x_k1_out, a.x_k1, sizeof(double) * (size_t)batch * nx, hipMemcpyDeviceToHost, sq));
        if (y_out && ny) HIP_TRY(hipMemcpyAsync(y_out, a.y, sizeof(double) * (size_t)batch * ny, hipMemcpyDeviceToHost, sq));
        if (cons_out && nc) HIP_TRY(hipMemcpyAsync(cons_out, a.cons, (size_t)batch * nc, hipMemcpyDeviceToHost, sq));
        if (cons_vio_out) HIP_TRY(hipMemcpyAsync(cons_vio_out, a.vio, sizeof(double) * batch, hipMemcpyDeviceToHost, sq));
        if (cons_row_out) HIP_TRY(hipMemcpyAsync(cons_row_out, a.row, sizeof(int) * batch, hipMemcpyDeviceToHost, sq));
        if (src.v0_out && nv) HIP_TRY(hipMemcpyAsync(src.v0_out, src.d_v0, sizeof(double) * (size_t)batch * nv, hipMemcpyDeviceToHost, sq));
        if (src.aux_status_out) HIP_TRY(hipMemcpyAsync(src.aux_status_out, src.d_auxst, sizeof(int) * batch, hipMemcpyDeviceToHost, sq));
        if (count_skipped) HIP_TRY(hipMemcpyAsync(&skipped, p->bat.skipped, sizeof(int), hipMemcpyDeviceToHost, sq));
        return MLD_OK;
    };
    if (int rc = queue_and_wait(sq, queue, wait)) return rc;
    /* queued without an error: the handle moves on */
    if (act_start) set_starts(p->pf_actual, std::move(d_start), batch, 1, gmax);
    if (log) ++L.count;
    if (advance) {
        std::swap(p->bat.x0, p->bat.x0b); std::swap(p->bat.omega, p->bat.omegab);
        if (plan || src.by_plan) inputs_advanced_by_plan(p); else inputs_advanced_by_caller(p);
    }
    if (n_skipped_out) *n_skipped_out = skipped;
    return MLD_OK;
}

int mld_sim_step_batch(mld_problem_t *p, const double *v0, const int64_t *act_start, int step, int flags,
                       double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out, int32_t *n_skipped_out)
{
    static const char who[] = "mld_sim_step_batch";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    std::vector<long long> gmax;
    if (int rc = sim_step_check(p, who, v0 != nullptr, "v0", act_start, step, flags, gmax)) return rc;
    if (!(flags & (MLD_SIM_ADVANCE | MLD_SIM_LOG)) && !x_k1_out && !y_out && !cons_out && !cons_vio_out && !cons_row_out && !n_skipped_out && !act_start) return MLD_OK;      /* nothing asked for */
    SimStepSrc src; src.v0 = v0;
    return sim_step_run(p, src, act_start, gmax, step, flags, x_k1_out, y_out, cons_out, cons_vio_out, cons_row_out, n_skipped_out);
}

/* Is `aux` the resolver of p's models -- their fold at N_tilde = 1, idle, without the hand-off -- or NULL exactly when there is nothing to resolve?
 * (mld_sim_step_resolve, mld_rollout_batch; `what`: the caller's word for p in the message) */
static int aux_fold_check(const char *who, const char *what, const mld_problem_t *p, const mld_problem_t *aux)
{
    const mld_dims &d = p->model->dims;
    const int nv2 = d.ndelta + d.nz + d.nmu;
    if (!nv2 && aux) { mld_set_error("%s: the model has no auxiliaries (ndelta + nz + nmu = 0), so there is nothing to resolve: aux must be NULL", who); return MLD_ERR_INVALID; }
    if (nv2 && !aux) { mld_set_error("%s: aux == NULL, but the model has %d auxiliaries to resolve (ndelta + nz + nmu)", who, nv2); return MLD_ERR_INVALID; }
    if (!aux) return MLD_OK;
    if (aux == p) { mld_set_error("%s: aux is the %s problem itself (the resolver is a handle of its own: the folded models at N_tilde = 1)", who, what); return MLD_ERR_INVALID; }
    if (aux->flight != Flight::idle) { mld_set_error("%s: aux has a launched solve that has not been finished (mld_solve_finish)", who); return MLD_ERR_INVALID; }
    if (aux->N != 1) { mld_set_error("%s: aux has N_tilde = %d (the auxiliary problem is the horizon-1 instance: N_tilde = 1)", who, aux->N); return MLD_ERR_INVALID; }
    if (aux->model->tv_N > 0) { mld_set_error("%s: aux is time-varying (mld_model_create_tv)", who); return MLD_ERR_INVALID; }
    if (aux->ho_enable) { mld_set_error("%s: aux has the in-kernel hand-off on (mld_set_handoff)", who); return MLD_ERR_INVALID; }
    const mld_dims &e = aux->model->dims;
    if (e.nx != d.nx || e.nc != d.nc || e.ndelta != d.ndelta || e.nz != d.nz || e.nmu != d.nmu || aux->n_models != p->n_models || e.nu != 0 || e.nomega != d.nomega + d.nu) {
        mld_set_error("%s: aux is not the fold of this problem's models: nx %d/%d nc %d/%d ndelta %d/%d nz %d/%d nmu %d/%d n_models %d/%d (aux/problem), nu %d (0), nomega %d (nomega + nu = %d)",
                      who, e.nx, d.nx, e.nc, d.nc, e.ndelta, d.ndelta, e.nz, d.nz, e.nmu, d.nmu, aux->n_models, p->n_models, e.nu, e.nomega, d.nomega + d.nu);
        return MLD_ERR_INVALID;
    }
    return MLD_OK;
}

/* ---- the plant step with the auxiliaries re-derived -------------------------------------------------------------------------------------------------
 * What the reference's closed loop really does: sim_step_k calls lsim_k(x_k=, u_k=, omega_k=) with u only, and lsim_k solves _compute_aux for delta, z, mu
 * under the REALISED omega_k before it forms x_k1, y and cons (controllers/controller_base.py:229-253, models/mld_model.py:683-686, 701-766).  `aux` is the
 * resolver's handle (aux_resolve.BatchAuxResolver: the folded models, N_tilde = 1, min sum(mu)); the call keeps no pointer to it.  Three phases, the host
 * waiting between them (the two handles may run on streams of their own): k_aux_inputs writes the resolver's inputs; the resolver's launch / finish solves
 * them; k_aux_merge builds v0 = [u; delta; z; mu] and k_sim_step steps on it.  Kernels: aux_step.inc.  p's inputs, log count and actual starts change only
 * when the last phase has been queued without an error.
 *
 * policy (mld_sim_step_policy): the same phases with one kernel in front -- k_policy_inputs writes the ruled channels of u, from the handle's current x0, the
 * resident u_prev and the policy tables, into the buffer the phases read u0 from; u0 / the resident plan supply the passed-through channels only, and no plan
 * is needed when every channel is ruled.  After an advancing step the resident u_prev of every ADVANCED instance becomes the u applied (k_policy_commit).
 *
 * fc (mld_sim_step_fallback, api_fallback.inc): the plan's step with one kernel in front -- k_fallback_inputs writes every instance's u from the first source
 * that applies (plan, plan memory, policy), its u_source and its attempt byte, which replaces the plan_usable test of the phases (AuxStepArgs::attempt).
 * After an advancing step k_policy_commit (a policy resident) and k_fallback_commit (a memory enabled) move the resident state on.
 *
 * fc->selected (mld_sim_step_selected, api_selected.inc): the same with the kept selection as the first source IN PLACE of the plan -- k_selected_inputs
 * and k_selected_commit (selected.inc) where the fallback step launches k_fallback_inputs and k_fallback_commit.  No channel of u is the resident plan's, so
 * the step needs no plan and leaves the handle as mld_sim_step_resolve(u0) does; the memory follows the advance as it follows the fallback step's. */
struct FallbackCall { int fb; int32_t *u_source_out; bool selected = false; int32_t *pick_out = nullptr; };

/* the (cap, batch) int array beside the log that one kind of step fills (SimLog::aux, SimLog::src): allocated by the first such step that logs, -2 elsewhere */
static int sim_log_side_array(mld_problem_t *p, DevBuf<int> &arr)
{
    if (arr) return MLD_OK;
    const size_t len = (size_t)p->slog.cap * p->batch;
    const hipStream_t sq = p->stream;
    DevBuf<int> la;
    HIP_TRY(la.alloc(len));
    auto fill = [&]() -> int { HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)la.get(), -2, len, sq)); return MLD_OK; };
    if (int rc = queue_and_wait(sq, fill)) return rc;
    arr = std::move(la);
    return MLD_OK;
}

static int sim_step_resolve_impl(const char *who, bool policy, mld_problem_t *p, mld_problem_t *aux, const double *u0, const int64_t *act_start, int step, int flags,
                                 double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out,
                                 double *v0_out, int32_t *aux_status_out, int32_t *n_skipped_out, const FallbackCall *fc = nullptr)
{
    if (policy && !p->pol_on) { mld_set_error("%s: no policy uploaded (mld_upload_policy)", who); return MLD_ERR_INVALID; }
    const bool selected = fc && fc->selected;
    const bool by_plan = !u0 && !(policy && p->pol_all_ruled) && !selected;      /* some channel of u is the resident plan's */
    std::vector<long long> gmax;
    if (int rc = sim_step_check(p, who, !by_plan, "u0", act_start, step, flags, gmax)) return rc;
    const mld_dims &d = p->model->dims;
    const int batch = p->batch, nx = d.nx, nu = d.nu, nw = d.nomega, nv = p->nv, nv2 = d.ndelta + d.nz + d.nmu;
    const bool actual = flags & MLD_SIM_ACTUAL, log = flags & MLD_SIM_LOG;
    if (int rc = aux_fold_check(who, "stepped", p, aux)) return rc;
    if (u0) for (size_t k = 0; k < (size_t)batch * nu; ++k) if (!std::isfinite(u0[k])) {
        mld_set_error("%s: u0 of instance %zu, input %zu is not finite (%g)", who, k / nu, k % nu, u0[k]); return MLD_ERR_INVALID;
    }
    if (!(flags & (MLD_SIM_ADVANCE | MLD_SIM_LOG)) && !x_k1_out && !y_out && !cons_out && !cons_vio_out && !cons_row_out && !v0_out && !aux_status_out && !n_skipped_out && !act_start && !(fc && (fc->u_source_out || fc->pick_out))) return MLD_OK;      /* nothing asked for */

    const hipStream_t sq = p->stream;
    mld_problem::SimLog &L = p->slog;
    if (log) { if (int rc = sim_log_side_array(p, L.aux)) return rc; }      /* every record so far was written by mld_sim_step_batch: "not resolved" */
    if (log && fc) { if (int rc = sim_log_side_array(p, L.src)) return rc; }
    if (log && selected) { if (int rc = sim_log_side_array(p, L.pick)) return rc; }
    const size_t log_slot = log ? (size_t)L.count * batch : 0;
    DevBuf<double> d_u, d_v0; DevBuf<unsigned char> d_mask, d_att; DevBuf<int> d_auxst, d_src, d_pick; DevBuf<long long> d_start;
    const bool commit_pol = policy || (fc && p->pol_on), commit_mem = fc && p->mem_on;      /* the resident state an advancing step moves on */
    if (commit_pol) { if (int rc = policy_state_ready(p, who)) return rc; }
    if (commit_mem) { if (int rc = plan_memory_ready(p, who)) return rc; }
    if (u0 || policy || fc) HIP_TRY(d_u.alloc((size_t)batch * std::max(1, nu)));
    if (fc) { HIP_TRY(d_att.alloc(batch)); HIP_TRY(d_src.alloc(batch)); }
    if (selected) HIP_TRY(d_pick.alloc(batch));
    if (act_start) HIP_TRY(d_start.alloc((size_t)batch * p->pf_groups));
    HIP_TRY(d_v0.alloc((size_t)batch * std::max(1, nv))); HIP_TRY(d_mask.alloc(batch)); HIP_TRY(d_auxst.alloc(batch));
    if (aux && (aux->batch != batch || aux->aux_src_gen != p->batch_gen || aux->aux_own_gen != aux->batch_gen)) {
        /* the resolver's resident batch: p's size, model_idx and hence RHS groups; its inputs are written on the device */
        std::vector<int32_t> midx;
        if (p->has_midx) { midx.resize(batch); HIP_TRY(hipMemcpy(midx.data(), p->bat.model_idx, sizeof(int) * batch, hipMemcpyDeviceToHost)); }
        if (int rc = lay_out_batch(aux, batch, p->has_midx ? midx.data() : nullptr, nullptr)) return rc;
        aux->aux_src_gen = p->batch_gen; aux->aux_own_gen = aux->batch_gen;
    }
    AuxStepArgs g{};
    g.batch = batch; g.nx = nx; g.nw = nw; g.nu = nu; g.nv = nv; g.nv2 = nv2; g.N = p->N;
    g.x0 = p->bat.x0; g.omega = p->bat.omega;
    if (u0 || policy || fc) { g.u = d_u; g.u_stride = (size_t)nu; }
    else { g.u = p->bat.v; g.u_stride = (size_t)p->n; }
    if (by_plan) { g.status = p->bat.status; g.obj = p->bat.obj; }
    FallbackArgs fa{};
    SelectedArgs sa{};
    if (selected) {
        g.attempt = d_att;
        sa.batch = batch; sa.nx = nx; sa.nu = nu; sa.N = p->N; sa.fb = fc->fb; sa.K = p->sel.K;
        sa.choice = p->sel.choice; sa.policy = p->sel.policy; sa.sel_u = p->sel.u;
        if (p->mem_on) { sa.mem_u = p->mem_u; sa.mem_age = p->mem_age; }
        if (p->pol_on) { sa.model_idx = p->has_midx ? p->bat.model_idx.get() : nullptr; sa.tab = p->pol_tab; sa.tab_len = (size_t)nu * (nx + POL_TAIL); sa.u_prev = p->pol_uprev; }
        sa.x0 = p->bat.x0; sa.u = d_u; sa.source = d_src; sa.pick = d_pick; sa.attempt = d_att;
    } else if (fc) {
        g.attempt = d_att;
        fa.batch = batch; fa.nx = nx; fa.nu = nu; fa.nv = nv; fa.N = p->N; fa.fb = fc->fb;
        fa.status = p->bat.status; fa.obj = p->bat.obj; fa.v = p->bat.v; fa.v_stride = (size_t)p->n;
        if (p->mem_on) { fa.mem_u = p->mem_u; fa.mem_age = p->mem_age; }
        if (p->pol_on) { fa.model_idx = p->has_midx ? p->bat.model_idx.get() : nullptr; fa.tab = p->pol_tab; fa.tab_len = (size_t)nu * (nx + POL_TAIL); fa.u_prev = p->pol_uprev; }
        fa.x0 = p->bat.x0; fa.u = d_u; fa.source = d_src; fa.attempt = d_att;
    }
    if (actual) { g.act_start = act_start ? d_start.get() : p->pf_actual.d.get(); g.chan = p->pf_chan; g.n_groups = p->pf_groups; g.step = step; g.lib = p->pf_lib; }
    /* ---- gather: the resolver's inputs -------------------------------------------------------------------------------------------------------------- */
    auto gather = [&]() -> int {
        if (u0 && nu) HIP_TRY(hipMemcpyAsync(d_u, u0, sizeof(double) * (size_t)batch * nu, hipMemcpyHostToDevice, sq));
        if (act_start) HIP_TRY(hipMemcpyAsync(d_start, act_start, sizeof(long long) * (size_t)batch * p->pf_groups, hipMemcpyHostToDevice, sq));
        if (policy && nu) {
            PolicyInputsArgs pa{};
            pa.batch = batch; pa.nx = nx; pa.nu = nu; pa.model_idx = p->has_midx ? p->bat.model_idx.get() : nullptr;
            pa.tab = p->pol_tab; pa.tab_len = (size_t)nu * (nx + POL_TAIL); pa.x0 = p->bat.x0; pa.u_prev = p->pol_uprev;
            if (by_plan) { pa.src = p->bat.v; pa.src_stride = (size_t)p->n; }
            pa.u = d_u;
            hipLaunchKernelGGL(k_policy_inputs, dim3(profile_grid((long long)batch * nu)), dim3(256), 0, sq, pa);
            HIP_TRY(hipGetLastError());
        }
        if (selected) {
            hipLaunchKernelGGL(k_selected_inputs, dim3(profile_grid((long long)batch * nu)), dim3(256), 0, sq, sa);
            HIP_TRY(hipGetLastError());
        } else if (fc) {
            hipLaunchKernelGGL(k_fallback_inputs, dim3(profile_grid((long long)batch * nu)), dim3(256), 0, sq, fa);
            HIP_TRY(hipGetLastError());
        }
        if (aux) {
            g.aux_x0 = aux->bat.x0; g.aux_omega = aux->bat.omega;
            hipLaunchKernelGGL(k_aux_inputs, dim3(profile_grid((long long)batch * (nx + nw + nu))), dim3(256), 0, sq, g);
            HIP_TRY(hipGetLastError());
        }
        return MLD_OK;
    };
    if (int rc = queue_and_wait(sq, gather)) return rc;
    /* ---- the auxiliary solve on the resolver's handle: new inputs, as after mld_select_inputs ----------------------------------------------------------- */
    if (aux) {
        inputs_replaced(aux);
        int rc = launch(aux);
        if (rc) { (void)hipStreamSynchronize(aux->stream); return rc; }
        if ((rc = finish(aux, nullptr))) return rc;
        g.aux_v = aux->bat.v; g.aux_stride = (size_t)aux->n; g.aux_status = aux->bat.status; g.aux_obj = aux->bat.obj;
    }
    /* ---- merge, then the step on the merged slices ----------------------------------------------------------------------------------------------------- */
    g.v0 = d_v0; g.usable = d_mask; g.aux_status_out = d_auxst;
    SimStepSrc src;
    src.merge = &g; src.d_v0 = d_v0; src.d_mask = d_mask; src.d_auxst = d_auxst; src.by_plan = by_plan; src.d_start = act_start ? &d_start : nullptr;
    src.v0_out = v0_out; src.aux_status_out = aux_status_out;
    int32_t skipped = 0;
    if (int rc = sim_step_run(p, src, act_start, gmax, step, flags, x_k1_out, y_out, cons_out, cons_vio_out, cons_row_out, &skipped)) return rc;
    if (n_skipped_out) *n_skipped_out = skipped;
    const bool advance = flags & MLD_SIM_ADVANCE;
    if ((commit_pol && advance && nu) || fc) {
        auto commit = [&]() -> int {
            if (fc && log) HIP_TRY(hipMemcpyAsync(L.src.get() + log_slot, d_src, sizeof(int) * batch, hipMemcpyDeviceToDevice, sq));
            if (fc && fc->u_source_out) HIP_TRY(hipMemcpyAsync(fc->u_source_out, d_src, sizeof(int) * batch, hipMemcpyDeviceToHost, sq));
            if (selected && log) HIP_TRY(hipMemcpyAsync(L.pick.get() + log_slot, d_pick, sizeof(int) * batch, hipMemcpyDeviceToDevice, sq));
            if (selected && fc->pick_out) HIP_TRY(hipMemcpyAsync(fc->pick_out, d_pick, sizeof(int) * batch, hipMemcpyDeviceToHost, sq));
            if (commit_pol && advance && nu) {
                hipLaunchKernelGGL(k_policy_commit, dim3(profile_grid((long long)batch * nu)), dim3(256), 0, sq, (long long)batch, nu, d_mask.get(), d_u.get(), p->pol_uprev.get());
                HIP_TRY(hipGetLastError());
            }
            if (commit_mem && advance) {
                if (selected) hipLaunchKernelGGL(k_selected_commit, dim3(profile_grid((long long)batch * p->N * nu)), dim3(256), 0, sq, sa);
                else hipLaunchKernelGGL(k_fallback_commit, dim3(profile_grid((long long)batch * p->N * nu)), dim3(256), 0, sq, fa);
                HIP_TRY(hipGetLastError());
            }
            return MLD_OK;
        };
        if (int rc = queue_and_wait(sq, commit)) return rc;
        if (commit_mem && advance) p->mem_chain = p->chain_gen;      /* the chain goes on: the advance counted as one more event, and the memory has followed it */
    }
    return MLD_OK;
}

int mld_sim_step_resolve(mld_problem_t *p, mld_problem_t *aux, const double *u0, const int64_t *act_start, int step, int flags,
                         double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out,
                         double *v0_out, int32_t *aux_status_out, int32_t *n_skipped_out)
{
    static const char who[] = "mld_sim_step_resolve";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    return sim_step_resolve_impl(who, false, p, aux, u0, act_start, step, flags, x_k1_out, y_out, cons_out, cons_vio_out, cons_row_out, v0_out, aux_status_out, n_skipped_out);
}

int mld_download_sim_log_aux(mld_problem_t *p, int first, int count, int32_t *aux_status)
{
    static const char who[] = "mld_download_sim_log_aux";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const mld_problem::SimLog &L = p->slog;
    if (first < 0 || count < 0 || (long long)first + count > L.count) { mld_set_error("%s: records [%d, %lld) asked for, %d logged", who, first, (long long)first + count, L.count); return MLD_ERR_INVALID; }
    if (count == 0 || !aux_status) return MLD_OK;
    const size_t off = (size_t)first * p->batch, len = (size_t)count * p->batch;
    if (!L.aux) { std::fill(aux_status, aux_status + len, -2); return MLD_OK; }      /* no resolving step has logged: every record is mld_sim_step_batch's */
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int { HIP_TRY(hipMemcpyAsync(aux_status, L.aux.get() + off, sizeof(int) * len, hipMemcpyDeviceToHost, sq)); return MLD_OK; };
    return queue_and_wait(sq, queue);
}

int mld_download_sim_log(mld_problem_t *p, int first, int count, double *x, double *v, double *y, double *omega, double *x_k1, uint8_t *cons, double *cons_vio,
                         int32_t *cons_row, double *obj, double *lower_bound, int32_t *status, int32_t *nodes)
{
    static const char who[] = "mld_download_sim_log";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
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
    return queue_and_wait(sq, queue);
}

} // extern "C"
