// Campaign KPIs (mld_sim_log_summary): column statistics of records [first, first + count) of the resident simulation log, reduced on the device by
// k_log_summary (log_summary.inc, where the rule is stated).  The call reads the log and writes nothing on the handle: everything it uploads and everything
// the kernel writes lives in temporaries of the call.  Every argument is tested on the host before anything is queued.
extern "C" {

int mld_sim_log_summary(mld_problem_t *p, int first, int count, int n_kpi,
                        const double *w_x, const double *w_v, const double *w_y, const double *w_omega, const double *w_xk1,
                        const int32_t *price_chan, const double *thresh, double vio_tol,
                        double *sum, double *min, double *max, int32_t *min_step, int32_t *max_step, int32_t *n_above, int32_t *n_changes,
                        int32_t *n_stepped, double *vio_max, int32_t *vio_step, int32_t *n_vio, int64_t *nodes_total, int32_t *n_source)
{
    static const char who[] = "mld_sim_log_summary";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const mld_problem::SimLog &L = p->slog;
    if (!L.cap) { mld_set_error("%s: no log has been begun for this batch (mld_sim_log_begin)", who); return MLD_ERR_INVALID; }
    if (first < 0 || count < 0 || (long long)first + count > L.count) { mld_set_error("%s: first, count: records [%d, %lld) asked for, %d logged", who, first, (long long)first + count, L.count); return MLD_ERR_INVALID; }
    if (n_kpi < 1 || n_kpi > MLD_KPI_MAX) { mld_set_error("%s: n_kpi = %d (1 .. MLD_KPI_MAX = %d)", who, n_kpi, MLD_KPI_MAX); return MLD_ERR_INVALID; }
    const mld_dims &d = p->model->dims;
    const int n_models = p->model->n_models, batch = p->batch, C = p->pr_chan;
    const double *tab[5] = {w_x, w_v, w_y, w_omega, w_xk1};
    const char *const names[5] = {"w_x", "w_v", "w_y", "w_omega", "w_xk1"};
    const int width[5] = {d.nx, p->nv, d.ny, d.nomega, d.nx};
    const double *fields[5] = {L.x, L.v, L.y, L.om, L.x_k1};
    if (!w_x && !w_v && !w_y && !w_omega && !w_xk1) { mld_set_error("%s: w_x, w_v, w_y, w_omega and w_xk1 are all NULL: a KPI needs a table", who); return MLD_ERR_INVALID; }
    if (d.nx < 1) { mld_set_error("%s: the model has no state (nx = 0): x_k1[0] marks the stepped records", who); return MLD_ERR_INVALID; }
    for (int t = 0; t < 5; ++t) {
        if (!tab[t]) continue;
        if (width[t] == 0) { mld_set_error("%s: %s given but the model has none of that variable (width 0)", who, names[t]); return MLD_ERR_INVALID; }
        const size_t len = (size_t)n_models * n_kpi * width[t];
        for (size_t i = 0; i < len; ++i) if (!std::isfinite(tab[t][i])) {
            mld_set_error("%s: %s of model %zu, KPI %zu, entry %zu is not finite (%g)", who, names[t], i / ((size_t)n_kpi * width[t]), i / width[t] % n_kpi, i % width[t], tab[t][i]);
            return MLD_ERR_INVALID;
        }
    }
    if (thresh) for (size_t i = 0; i < (size_t)n_models * n_kpi; ++i) if (std::isnan(thresh[i])) {
        mld_set_error("%s: thresh of model %zu, KPI %zu is NaN", who, i / n_kpi, i % n_kpi); return MLD_ERR_INVALID;
    }
    if (std::isnan(vio_tol)) { mld_set_error("%s: vio_tol is NaN", who); return MLD_ERR_INVALID; }
    bool priced = false;
    if (price_chan) for (int q = 0; q < n_kpi; ++q) {
        const int c = price_chan[q];
        if (c < -1) { mld_set_error("%s: price_chan[%d] = %d (-1 = not priced, or a channel 0 .. n_chan - 1)", who, q, c); return MLD_ERR_INVALID; }
        if (c >= 0 && !L.cost) { mld_set_error("%s: price_chan[%d] = %d, but no stage cost is armed for the resident log (mld_sim_log_cost_begin): there is no price record", who, q, c); return MLD_ERR_INVALID; }
        if (c >= C) { mld_set_error("%s: price_chan[%d] = %d, but the price library has n_chan = %d", who, q, c, C); return MLD_ERR_INVALID; }
        priced = priced || c >= 0;
    }
    /* what a record stages: the given tables' fields, element 0 of x_k1 where w_xk1 is not given, the price record where a KPI is priced */
    LogSummaryArgs a{};
    a.batch = batch; a.first = first; a.count = count; a.n_kpi = n_kpi; a.vio_tol = vio_tol;
    int off = 0;
    for (int t = 0; t < 5; ++t) if (tab[t]) { a.seg[a.n_seg++] = LsSeg{fields[t], width[t], width[t], off}; off += width[t]; }
    a.n_fun = a.n_seg; a.rows = off;
    if (w_xk1) a.flag_off = a.seg[a.n_seg - 1].off;
    else { a.flag_off = off; a.seg[a.n_seg++] = LsSeg{L.x_k1, d.nx, 1, off}; off += 1; }
    a.price_off = -1;
    if (priced) { a.price_off = off; a.seg[a.n_seg++] = LsSeg{L.price, C, C, off}; off += C; }
    a.staged = off;
    a.prefetch = off <= 64 * LS_SLOTS && !(p->opts.reserved & MLD_DBG_SUMMARY_NO_PREFETCH);
    const size_t lds = sizeof(double) * LS_WAVES * 2 * (size_t)off;
    if (lds > LS_LDS_MAX) { mld_set_error("%s: a record of %d staged doubles does not fit the staging of k_log_summary (%zu bytes of LDS)", who, off, (size_t)LS_LDS_MAX); return MLD_ERR_INVALID; }
    /* the tables side by side, KPI-minor: W[m, row, q] */
    const size_t nq = (size_t)n_models * n_kpi, bq = (size_t)batch * n_kpi;
    std::vector<double> hW((size_t)n_models * a.rows * n_kpi), hthr(nq, std::numeric_limits<double>::infinity());
    std::vector<int> hpc(n_kpi, -1);
    for (int m = 0; m < n_models; ++m) {
        int row = 0;
        for (int t = 0; t < 5; ++t) {
            if (!tab[t]) continue;
            for (int q = 0; q < n_kpi; ++q)
                for (int i = 0; i < width[t]; ++i) hW[((size_t)m * a.rows + row + i) * n_kpi + q] = tab[t][((size_t)m * n_kpi + q) * width[t] + i];
            row += width[t];
        }
    }
    if (thresh) std::copy(thresh, thresh + nq, hthr.begin());
    if (price_chan) std::copy(price_chan, price_chan + n_kpi, hpc.begin());
    DevBuf<double> d_W, d_thr, d_sum, d_min, d_max, d_vmax; DevBuf<int> d_pc, d_mins, d_maxs, d_above, d_chg, d_nst, d_vstep, d_nvio, d_nsrc; DevBuf<long long> d_nodes;
    HIP_TRY(d_W.alloc(hW.size())); HIP_TRY(d_thr.alloc(nq)); HIP_TRY(d_pc.alloc(n_kpi));
    HIP_TRY(d_sum.alloc(bq)); HIP_TRY(d_min.alloc(bq)); HIP_TRY(d_max.alloc(bq)); HIP_TRY(d_mins.alloc(bq)); HIP_TRY(d_maxs.alloc(bq)); HIP_TRY(d_above.alloc(bq)); HIP_TRY(d_chg.alloc(bq));
    HIP_TRY(d_nst.alloc(batch)); HIP_TRY(d_vmax.alloc(batch)); HIP_TRY(d_vstep.alloc(batch)); HIP_TRY(d_nvio.alloc(batch)); HIP_TRY(d_nodes.alloc(batch)); HIP_TRY(d_nsrc.alloc((size_t)batch * 3));
    a.model_idx = p->has_midx ? p->bat.model_idx.get() : nullptr;
    a.W = d_W; a.thresh = d_thr; a.price_chan = d_pc;
    a.vio = L.vio; a.nodes = L.nodes; a.source = L.src ? L.src.get() : nullptr;
    a.sum = d_sum; a.min = d_min; a.max = d_max; a.min_step = d_mins; a.max_step = d_maxs; a.n_above = d_above; a.n_changes = d_chg;
    a.n_stepped = d_nst; a.vio_max = d_vmax; a.vio_step = d_vstep; a.n_vio = d_nvio; a.nodes_total = d_nodes; a.n_source = d_nsrc;
    int dev = 0, per_cu = 0; hipDeviceProp_t prop;
    (void)hipGetDevice(&dev); HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_log_summary, 64 * LS_WAVES, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    const int grid = (int)std::min<long long>(((long long)batch + LS_WAVES - 1) / LS_WAVES, (long long)per_cu * prop.multiProcessorCount);
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_W, hW.data(), sizeof(double) * hW.size(), hipMemcpyHostToDevice, sq));
        HIP_TRY(hipMemcpyAsync(d_thr, hthr.data(), sizeof(double) * nq, hipMemcpyHostToDevice, sq));
        HIP_TRY(hipMemcpyAsync(d_pc, hpc.data(), sizeof(int) * n_kpi, hipMemcpyHostToDevice, sq));
        hipLaunchKernelGGL(k_log_summary, dim3(grid), dim3(64 * LS_WAVES), lds, sq, a);
        HIP_TRY(hipGetLastError());
        auto get = [&](void *dst, const void *src, size_t bytes) -> hipError_t { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, sq) : hipSuccess; };
        HIP_TRY(get(sum, d_sum, sizeof(double) * bq)); HIP_TRY(get(min, d_min, sizeof(double) * bq)); HIP_TRY(get(max, d_max, sizeof(double) * bq));
        HIP_TRY(get(min_step, d_mins, sizeof(int) * bq)); HIP_TRY(get(max_step, d_maxs, sizeof(int) * bq));
        HIP_TRY(get(n_above, d_above, sizeof(int) * bq)); HIP_TRY(get(n_changes, d_chg, sizeof(int) * bq));
        HIP_TRY(get(n_stepped, d_nst, sizeof(int) * batch)); HIP_TRY(get(vio_max, d_vmax, sizeof(double) * batch)); HIP_TRY(get(vio_step, d_vstep, sizeof(int) * batch));
        HIP_TRY(get(n_vio, d_nvio, sizeof(int) * batch)); HIP_TRY(get(nodes_total, d_nodes, sizeof(long long) * batch)); HIP_TRY(get(n_source, d_nsrc, sizeof(int) * (size_t)batch * 3));
        return MLD_OK;
    };
    return queue_and_wait(sq, queue);
}

} // extern "C"
