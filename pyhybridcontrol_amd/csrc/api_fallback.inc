// Fallback inputs for instances without a usable plan (mld_plan_memory, mld_set_plan_memory, mld_download_plan_memory, mld_sim_step_fallback,
// mld_download_sim_log_source): the resolving plant step with the source of u chosen per instance on the device -- the resident plan, the remembered plan's
// row for the current time, or the resident policy's rule -- where the reference goes on with "the last solution" (examples/
// residential_mg_with_pv_and_dewhs/modelling/micro_grid_agents.py:728-735, controllers/controller_base.py:229-253).  The step is sim_step_resolve_impl's body
// (api_resident.inc) with the fallback switched on; kernels: k_fallback_inputs, k_fallback_commit (fallback.inc).
extern "C" {

int mld_plan_memory(mld_problem_t *p, int enable)
{
    static const char who[] = "mld_plan_memory";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch): the memory belongs to a batch")) return rc;
    if (!enable) { p->mem_u.reset(); p->mem_age.reset(); p->mem_on = false; p->mem_batch_gen = 0; return MLD_OK; }
    if (p->model->dims.nu < 1) { mld_set_error("%s: the model has no input (nu = 0): there is nothing to remember", who); return MLD_ERR_INVALID; }
    const bool was_on = p->mem_on;
    const unsigned long long was_gen = p->mem_batch_gen;
    p->mem_on = true; p->mem_batch_gen = 0;      /* laid out anew, and empty */
    if (int rc = plan_memory_ready(p, who)) { p->mem_on = was_on; p->mem_batch_gen = was_gen; return rc; }
    return MLD_OK;
}

int mld_set_plan_memory(mld_problem_t *p, const double *u, const int32_t *age)
{
    static const char who[] = "mld_set_plan_memory";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    if (!p->mem_on) { mld_set_error("%s: no plan memory enabled (mld_plan_memory)", who); return MLD_ERR_INVALID; }
    const int N = p->N, nu = p->model->dims.nu;
    const size_t batch = (size_t)p->batch, row = (size_t)N * nu, len = batch * row;
    if (u) for (size_t k = 0; k < len; ++k) if (!std::isfinite(u[k])) {
        mld_set_error("%s: u of instance %zu, step %zu, input %zu is not finite (%g)", who, k / row, k % row / nu, k % nu, u[k]); return MLD_ERR_INVALID;
    }
    if (age) for (size_t b = 0; b < batch; ++b) if (age[b] != -1 && (age[b] < 1 || age[b] > N)) {
        mld_set_error("%s: age of instance %zu is %d (-1 = nothing remembered, or 1 .. N_tilde = %d)", who, b, (int)age[b], N); return MLD_ERR_INVALID;
    }
    if (int rc = plan_memory_ready(p, who)) return rc;
    if (!u && !age) return MLD_OK;
    /* staged beside the resident arrays and swapped in once both have arrived: a call that fails changes nothing */
    const hipStream_t sq = p->stream;
    DevBuf<double> d_u; DevBuf<int> d_age;
    if (u) HIP_TRY(d_u.alloc(len));
    if (age) HIP_TRY(d_age.alloc(batch));
    auto stage = [&]() -> int {
        if (u) HIP_TRY(hipMemcpyAsync(d_u, u, sizeof(double) * len, hipMemcpyHostToDevice, sq));
        if (age) HIP_TRY(hipMemcpyAsync(d_age, age, sizeof(int) * batch, hipMemcpyHostToDevice, sq));
        return MLD_OK;
    };
    if (int rc = queue_and_wait(sq, stage)) return rc;
    if (u) p->mem_u = std::move(d_u);
    if (age) p->mem_age = std::move(d_age);
    return MLD_OK;
}

int mld_download_plan_memory(mld_problem_t *p, double *u_out, int32_t *age_out)
{
    static const char who[] = "mld_download_plan_memory";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    if (int rc = plan_memory_ready(p, who)) return rc;
    const hipStream_t sq = p->stream;
    const size_t batch = (size_t)p->batch, len = batch * p->N * p->model->dims.nu;
    auto queue = [&]() -> int {
        if (u_out) HIP_TRY(hipMemcpyAsync(u_out, p->mem_u.get(), sizeof(double) * len, hipMemcpyDeviceToHost, sq));
        if (age_out) HIP_TRY(hipMemcpyAsync(age_out, p->mem_age.get(), sizeof(int) * batch, hipMemcpyDeviceToHost, sq));
        return MLD_OK;
    };
    return queue_and_wait(sq, queue);
}

int mld_sim_step_fallback(mld_problem_t *p, mld_problem_t *aux, int fb, const int64_t *act_start, int step, int flags,
                          double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out,
                          double *v0_out, int32_t *aux_status_out, int32_t *u_source_out, int32_t *n_skipped_out)
{
    static const char who[] = "mld_sim_step_fallback";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    if (fb & ~(MLD_FB_MEMORY | MLD_FB_POLICY)) { mld_set_error("%s: unknown fallback bits 0x%x (MLD_FB_MEMORY | MLD_FB_POLICY)", who, fb); return MLD_ERR_INVALID; }
    if (p->model->dims.nu < 1) { mld_set_error("%s: the model has no input (nu = 0): there is no u a fallback could supply", who); return MLD_ERR_INVALID; }
    if ((fb & MLD_FB_MEMORY) && !p->mem_on) { mld_set_error("%s: MLD_FB_MEMORY, but no plan memory is enabled (mld_plan_memory)", who); return MLD_ERR_INVALID; }
    if ((fb & MLD_FB_POLICY) && !p->pol_on) { mld_set_error("%s: MLD_FB_POLICY, but no policy uploaded (mld_upload_policy)", who); return MLD_ERR_INVALID; }
    if ((fb & MLD_FB_POLICY) && !p->pol_all_ruled) {
        mld_set_error("%s: MLD_FB_POLICY, but the resident policy passes a channel through (mode 0): an instance without a usable plan has no u such a channel could take", who);
        return MLD_ERR_INVALID;
    }
    const FallbackCall fc{fb, u_source_out};
    return sim_step_resolve_impl(who, false, p, aux, nullptr, act_start, step, flags, x_k1_out, y_out, cons_out, cons_vio_out, cons_row_out, v0_out, aux_status_out,
                                 n_skipped_out, &fc);
}

int mld_download_sim_log_source(mld_problem_t *p, int first, int count, int32_t *u_source)
{
    static const char who[] = "mld_download_sim_log_source";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const mld_problem::SimLog &L = p->slog;
    if (first < 0 || count < 0 || (long long)first + count > L.count) { mld_set_error("%s: records [%d, %lld) asked for, %d logged", who, first, (long long)first + count, L.count); return MLD_ERR_INVALID; }
    if (count == 0 || !u_source) return MLD_OK;
    const size_t off = (size_t)first * p->batch, len = (size_t)count * p->batch;
    if (!L.src) { std::fill(u_source, u_source + len, -2); return MLD_OK; }      /* no fallback step has logged: every record is another entry point's */
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int { HIP_TRY(hipMemcpyAsync(u_source, L.src.get() + off, sizeof(int) * len, hipMemcpyDeviceToHost, sq)); return MLD_OK; };
    return queue_and_wait(sq, queue);
}

} // extern "C"
