// Resident price profiles (prices.inc): the price library, the per-instance cost of a resident batch from price windows (k_price_cost, then the tail of
// mld_upload_instance_cost), and the stage cost in the simulation log (armed here, written by k_stage_cost behind every logged step: sim_step_run).  Every
// start is tested on the host before anything is queued (check_starts / check_resident, the pieces of the disturbance library's window rule, over the price
// library as ONE group of width n_chan); everything new is built beside what is resident and moved in once the stream has taken it.
extern "C" {

static void drop_price_tables(mld_problem *p)
{
    p->pr_tab.reset(); p->sc_tab.reset(); p->pr_tab_on = p->pr_ay = p->sc_on = false;
}

int mld_upload_prices(mld_problem_t *p, int64_t lib_len, const double *lib, int n_chan)
{
    static const char who[] = "mld_upload_prices";
    if (int rc = entry_guard(p, who, true, nullptr)) return rc;
    if (!p) { mld_set_error("%s: null problem", who); return MLD_ERR_INVALID; }
    if (lib_len < 0 || (lib_len > 0 && !lib)) { mld_set_error("%s: lib_len = %lld%s", who, (long long)lib_len, lib_len > 0 ? " without a library" : ""); return MLD_ERR_INVALID; }
    if (lib_len == 0) {      /* frees the library; the starts, the tables shaped by its n_chan and an armed stage cost go with it */
        p->pr_lib.reset(); p->pr_len = 0; p->pr_chan = 0; p->pr_cost.reset(); drop_price_tables(p); p->slog.disarm();
        return MLD_OK;
    }
    if (n_chan < 1) { mld_set_error("%s: n_chan = %d (a price series has at least one channel)", who, n_chan); return MLD_ERR_INVALID; }
    if (price_stage_doubles(p->N, n_chan) * sizeof(double) > PC_LDS_MAX) {
        mld_set_error("%s: n_chan = %d: a window and its sums, (N_tilde + 1) x n_chan = %zu doubles, do not fit the %zu bytes k_price_cost stages a row in", who, n_chan,
                      price_stage_doubles(p->N, n_chan), (size_t)PC_LDS_MAX);
        return MLD_ERR_INVALID;
    }
    DevBuf<double> d_lib;      /* built beside the resident library: a call that fails leaves it as it was */
    HIP_TRY(d_lib.alloc((size_t)lib_len));
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int { HIP_TRY(hipMemcpyAsync(d_lib, lib, sizeof(double) * (size_t)lib_len, hipMemcpyHostToDevice, sq)); return MLD_OK; };
    if (int rc = queue_and_wait(sq, queue)) return rc;
    if (n_chan != p->pr_chan) drop_price_tables(p);      /* they were shaped by the n_chan that is gone */
    p->pr_lib = std::move(d_lib); p->pr_len = lib_len; p->pr_chan = n_chan;
    p->pr_cost.reset(); p->slog.disarm();      /* the starts pointed into the library that is gone */
    return MLD_OK;
}

/* per-model tables (n_models, n_chan, width) laid end to end into one device buffer, zeros where the caller gave none; a non-finite entry is named */
struct PriceTable { const char *name; const double *src; int width; };
static int upload_price_tables(mld_problem *p, const char *who, const PriceTable *t, int n_tab, DevBuf<double> &out)
{
    const size_t MC = (size_t)p->n_models * p->pr_chan;
    size_t len = 0;
    for (int k = 0; k < n_tab; ++k) len += MC * t[k].width;
    std::vector<double> tab(len, 0.0);
    size_t off = 0;
    for (int k = 0; k < n_tab; ++k) {
        const size_t w = t[k].width;
        if (t[k].src) for (size_t e = 0; e < MC * w; ++e) {
            if (!std::isfinite(t[k].src[e])) {
                mld_set_error("%s: %s of model %zu, channel %zu, column %zu is not finite (%g)", who, t[k].name, e / w / p->pr_chan, e / w % p->pr_chan, e % w, t[k].src[e]);
                return MLD_ERR_INVALID;
            }
            tab[off + e] = t[k].src[e];
        }
        off += MC * w;
    }
    DevBuf<double> d;
    HIP_TRY(d.alloc(len));
    if (len) HIP_TRY(hipMemcpy(d, tab.data(), sizeof(double) * len, hipMemcpyHostToDevice));
    out = std::move(d);
    return MLD_OK;
}

int mld_set_price_cost(mld_problem_t *p, const double *a_v, const double *sum_v, const double *a_y)
{
    static const char who[] = "mld_set_price_cost";
    if (int rc = entry_guard(p, who, true, nullptr)) return rc;
    if (!p) { mld_set_error("%s: null problem", who); return MLD_ERR_INVALID; }
    if (!a_v && !sum_v && !a_y) { p->pr_tab.reset(); p->pr_tab_on = p->pr_ay = false; return MLD_OK; }
    if (!p->pr_len) { mld_set_error("%s: no price library resident (mld_upload_prices): its n_chan shapes the tables", who); return MLD_ERR_INVALID; }
    const int ny = p->model->dims.ny;
    if (a_y && ny == 0) { mld_set_error("%s: a_y given but the model has no output (ny = 0)", who); return MLD_ERR_INVALID; }
    const PriceTable t[3] = {{"a_v", a_v, p->nv}, {"sum_v", sum_v, p->nv}, {"a_y", a_y, ny}};
    if (int rc = upload_price_tables(p, who, t, 3, p->pr_tab)) return rc;
    p->pr_tab_on = true; p->pr_ay = a_y != nullptr;
    return MLD_OK;
}

int mld_instance_cost_from_prices(mld_problem_t *p, const int64_t *start, int step)
{
    static const char who[] = "mld_instance_cost_from_prices";
    if (int rc = entry_guard(p, who, true, "upload a batch first (the cost belongs to its instances)")) return rc;
    if (!p->pr_len) { mld_set_error("%s: no price library resident (mld_upload_prices)", who); return MLD_ERR_INVALID; }
    if (!p->pr_tab_on) { mld_set_error("%s: no price tables set (mld_set_price_cost)", who); return MLD_ERR_INVALID; }
    if (step < 0 || step > INT_MAX - p->N) { mld_set_error("%s: step = %d (must be >= 0)", who, step); return MLD_ERR_INVALID; }
    if (p->model->tv_N > 0) { mld_set_error("%s: time-varying models (mld_model_create_tv) take their per-instance cost from the host (mld_upload_instance_cost): the tables are per model, not per step model", who); return MLD_ERR_INVALID; }
    const int n = p->n, nv = p->nv, N = p->N, batch = p->batch, C = p->pr_chan, ny = p->model->dims.ny;
    const int NX = N * p->model->dims.nx, NY = N * ny, K = NX + NY;
    std::vector<long long> gmax;
    if (start) { if (int rc = check_starts(price_lib(p), who, PF_PRICE, start, batch, 1, step, N, gmax)) return rc; }
    else {
        if (p->pr_cost.batch != batch) { mld_set_error("%s: start == NULL, but no price starts of this batch are resident (pass them once)", who); return MLD_ERR_INVALID; }
        if (int rc = check_resident(price_lib(p), who, PF_PRICE, p->pr_cost.gmax, step, N)) return rc;
    }
    const hipStream_t sq = p->stream;
    const bool pull = p->pr_ay;
    const int ld = inst_cost_ld(p, pull);
    DevBuf<double> ic, d_w; DevBuf<long long> d_start;
    HIP_TRY(ic.alloc((size_t)batch * std::max(1, ld)));
    if (pull) HIP_TRY(d_w.alloc((size_t)batch * K));
    if (start) HIP_TRY(d_start.alloc(batch));
    PriceCostArgs a{};
    a.batch = batch; a.N = N; a.n_chan = C; a.step = step;
    a.rpw = (int)std::max<size_t>(1, std::min<size_t>(PC_WAVES, PC_LDS_MAX / (price_stage_doubles(N, C) * sizeof(double))));
    a.model_idx = p->has_midx ? p->bat.model_idx.get() : nullptr;
    a.start = start ? d_start.get() : p->pr_cost.d.get(); a.lib = p->pr_lib;
    const size_t tab = (size_t)p->n_models * C * nv, lds = sizeof(double) * a.rpw * price_stage_doubles(N, C);
    const int grid = (int)std::max<long long>(1, std::min<long long>(((long long)batch + a.rpw - 1) / a.rpw, 8192));      /* bounded: the rest is the grid-stride loop */
    /* the cost is built in a buffer of its own and every path waits for the stream (queue_and_wait): a call that fails leaves the resident cost as it was */
    auto queue = [&]() -> int {
        if (start) HIP_TRY(hipMemcpyAsync(d_start, start, sizeof(long long) * (size_t)batch, hipMemcpyHostToDevice, sq));
        if (pull) HIP_TRY(hipMemsetAsync(ic, 0, sizeof(double) * (size_t)batch * std::max(1, ld), sq));      /* cx / cw / c0: the GEMM accumulates into them */
        if (n) {
            a.W = nv; a.a = p->pr_tab; a.s = p->pr_tab.get() + tab; a.dst = ic; a.ld = (size_t)ld;
            hipLaunchKernelGGL(k_price_cost, dim3(grid), dim3(64 * PC_WAVES), lds, sq, a);
            HIP_TRY(hipGetLastError());
        }
        if (pull) {
            HIP_TRY(hipMemsetAsync(d_w, 0, sizeof(double) * (size_t)batch * K, sq));      /* no weights on x_tilde */
            a.W = ny; a.a = p->pr_tab.get() + 2 * tab; a.s = nullptr; a.dst = d_w.get() + NX; a.ld = (size_t)K;
            hipLaunchKernelGGL(k_price_cost, dim3(grid), dim3(64 * PC_WAVES), lds, sq, a);
            HIP_TRY(hipGetLastError());
            if (int rc = queue_inst_pullback(p, sq, d_w.get(), ic.get())) return rc;
        }
        return MLD_OK;
    };
    if (int rc = queue_and_wait(sq, queue)) return rc;
    adopt_inst_cost(p, std::move(ic), ld);
    if (start) set_starts(p->pr_cost, std::move(d_start), batch, 1, gmax);
    return MLD_OK;
}

int mld_set_stage_cost(mld_problem_t *p, const double *w_v, const double *w_y)
{
    static const char who[] = "mld_set_stage_cost";
    if (int rc = entry_guard(p, who, true, nullptr)) return rc;
    if (!p) { mld_set_error("%s: null problem", who); return MLD_ERR_INVALID; }
    if (!w_v && !w_y) { p->sc_tab.reset(); p->sc_on = false; p->slog.disarm(); return MLD_OK; }      /* without weights there is no stage cost to log */
    if (!p->pr_len) { mld_set_error("%s: no price library resident (mld_upload_prices): its n_chan shapes the tables", who); return MLD_ERR_INVALID; }
    const int ny = p->model->dims.ny;
    if (w_y && ny == 0) { mld_set_error("%s: w_y given but the model has no output (ny = 0)", who); return MLD_ERR_INVALID; }
    if (p->slog.cost) HIP_TRY(hipStreamSynchronize(p->stream));      /* a logged step still in flight reads the tables that go */
    const PriceTable t[2] = {{"w_v", w_v, p->nv}, {"w_y", w_y, ny}};
    if (int rc = upload_price_tables(p, who, t, 2, p->sc_tab)) return rc;
    p->sc_on = true;
    return MLD_OK;
}

int mld_sim_log_cost_begin(mld_problem_t *p, const int64_t *start)
{
    static const char who[] = "mld_sim_log_cost_begin";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch): the log belongs to a batch")) return rc;
    mld_problem::SimLog &L = p->slog;
    if (!L.cap) { mld_set_error("%s: no log has been begun for this batch (mld_sim_log_begin)", who); return MLD_ERR_INVALID; }
    if (!p->pr_len) { mld_set_error("%s: no price library resident (mld_upload_prices)", who); return MLD_ERR_INVALID; }
    if (!p->sc_on) { mld_set_error("%s: no stage weights set (mld_set_stage_cost)", who); return MLD_ERR_INVALID; }
    if (!start) { mld_set_error("%s: start == NULL (the starts of the realised prices, one per instance)", who); return MLD_ERR_INVALID; }
    const int batch = p->batch, C = p->pr_chan;
    std::vector<long long> gmax;
    if (int rc = check_starts(price_lib(p), who, PF_PRICE_ELEMENT, start, batch, 1, 0, 1, gmax)) return rc;
    const size_t cb = (size_t)L.cap * (size_t)batch;
    if (cb > SIZE_MAX / sizeof(double) / (size_t)C) { mld_set_error("%s: capacity %d x batch %d x n_chan %d entries does not fit size_t", who, L.cap, batch, C); return MLD_ERR_INVALID; }
    DevBuf<double> cost, price, total; DevBuf<int> steps; DevBuf<long long> d_start;      /* built beside an armed stage cost: a call that fails leaves it as it was */
    HIP_TRY(cost.alloc(cb)); HIP_TRY(price.alloc(cb * C)); HIP_TRY(total.alloc(batch)); HIP_TRY(steps.alloc(batch)); HIP_TRY(d_start.alloc(batch));
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int {
        const double qnan = std::numeric_limits<double>::quiet_NaN();
        hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)((cb + 255) / 256)), dim3(256), 0, sq, cb, qnan, cost.get());
        hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)((cb * C + 255) / 256)), dim3(256), 0, sq, cb * C, qnan, price.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(total, 0, sizeof(double) * batch, sq));
        HIP_TRY(hipMemsetAsync(steps, 0, sizeof(int) * batch, sq));
        HIP_TRY(hipMemcpyAsync(d_start, start, sizeof(long long) * (size_t)batch, hipMemcpyHostToDevice, sq));
        return MLD_OK;
    };
    if (int rc = queue_and_wait(sq, queue)) return rc;
    L.cost = std::move(cost); L.price = std::move(price); L.total = std::move(total); L.steps = std::move(steps); L.cstart = std::move(d_start);
    L.cstart_max = gmax[0];
    return MLD_OK;
}

int mld_download_sim_log_cost(mld_problem_t *p, int first, int count, double *cost, double *price)
{
    static const char who[] = "mld_download_sim_log_cost";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const mld_problem::SimLog &L = p->slog;
    if (!L.cost) { mld_set_error("%s: no stage cost is armed for the resident log (mld_sim_log_cost_begin)", who); return MLD_ERR_INVALID; }
    if (first < 0 || count < 0 || (long long)first + count > L.count) { mld_set_error("%s: records [%d, %lld) asked for, %d logged", who, first, (long long)first + count, L.count); return MLD_ERR_INVALID; }
    if (count == 0) return MLD_OK;
    const size_t off = (size_t)first * p->batch, len = (size_t)count * p->batch, C = (size_t)p->pr_chan;
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int {
        if (cost) HIP_TRY(hipMemcpyAsync(cost, L.cost.get() + off, sizeof(double) * len, hipMemcpyDeviceToHost, sq));
        if (price) HIP_TRY(hipMemcpyAsync(price, L.price.get() + off * C, sizeof(double) * len * C, hipMemcpyDeviceToHost, sq));
        return MLD_OK;
    };
    return queue_and_wait(sq, queue);
}

int mld_download_cost_total(mld_problem_t *p, double *total, int32_t *steps)
{
    static const char who[] = "mld_download_cost_total";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const mld_problem::SimLog &L = p->slog;
    if (!L.cost) { mld_set_error("%s: no stage cost is armed for the resident log (mld_sim_log_cost_begin)", who); return MLD_ERR_INVALID; }
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int {
        if (total) HIP_TRY(hipMemcpyAsync(total, L.total.get(), sizeof(double) * p->batch, hipMemcpyDeviceToHost, sq));
        if (steps) HIP_TRY(hipMemcpyAsync(steps, L.steps.get(), sizeof(int) * p->batch, hipMemcpyDeviceToHost, sq));
        return MLD_OK;
    };
    return queue_and_wait(sq, queue);
}

} // extern "C"
