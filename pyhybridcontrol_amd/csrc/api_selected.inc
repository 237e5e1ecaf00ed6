// Applying a selection on the device (mld_keep_selection, mld_set_selection, mld_download_selection, mld_sim_step_selected, mld_download_sim_log_pick):
// mld_rollout_select / mld_rollout_select_policy are the safety filter in front of the plant step, and this is the step behind it -- the chosen inputs stay
// where they were chosen, the plan memory and the policy state follow the input that was applied, and the log says which candidate that was.  The step is
// sim_step_resolve_impl's body (api_resident.inc) with the kept selection as the first source in place of the plan; kernels: k_selected_inputs,
// k_selected_commit (selected.inc).  The kept copy itself is made by rollout_impl (api_rollout.inc: keep_selection).
extern "C" {

int mld_keep_selection(mld_problem_t *p, int enable)
{
    static const char who[] = "mld_keep_selection";
    if (!p) { mld_set_error("%s: p is NULL", who); return MLD_ERR_INVALID; }
    if (p->flight != Flight::idle) { mld_set_error("%s: a launched solve has not been finished (mld_solve_finish)", who); return MLD_ERR_INVALID; }
    p->sel_keep = enable != 0;
    if (!enable) p->sel = mld_problem::Selection();
    return MLD_OK;
}

int mld_set_selection(mld_problem_t *p, int K, const int32_t *choice, const int32_t *policy, const double *u)
{
    static const char who[] = "mld_set_selection";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch): a selection belongs to a batch")) return rc;
    const int nu = p->model->dims.nu;
    if (nu < 1) { mld_set_error("%s: the model has no input (nu = 0): there is nothing to select", who); return MLD_ERR_INVALID; }
    if (K < 1) { mld_set_error("%s: K = %d (the steps of a chosen sequence: at least 1)", who, K); return MLD_ERR_INVALID; }
    if (!choice || !u) { mld_set_error("%s: %s is NULL (choice (batch), u (batch, K, nu); policy may be NULL: every pick a sequence)", who, !choice ? "choice" : "u"); return MLD_ERR_INVALID; }
    const size_t batch = (size_t)p->batch, row = (size_t)K * nu;
    for (size_t b = 0; b < batch; ++b) {
        const int pol = policy ? policy[b] : -1;
        if (choice[b] < -1) { mld_set_error("%s: choice of instance %zu is %d (-1 = none, or a candidate >= 0)", who, b, (int)choice[b]); return MLD_ERR_INVALID; }
        if (pol < -1) { mld_set_error("%s: policy of instance %zu is %d (-1 = a plan or sequence pick or none, or a policy >= 0)", who, b, pol); return MLD_ERR_INVALID; }
        if (choice[b] < 0 && pol >= 0) { mld_set_error("%s: policy of instance %zu is %d, but its choice is -1 (no pick has no policy)", who, b, pol); return MLD_ERR_INVALID; }
        if (choice[b] < 0) continue;      /* no choice: its rows are not read (the select calls leave NaN there) */
        const size_t rows = pol < 0 ? row : (size_t)nu;      /* a policy pick has its step 0 only */
        for (size_t e = 0; e < rows; ++e) if (!std::isfinite(u[b * row + e])) {
            mld_set_error("%s: u of instance %zu, step %zu, input %zu is not finite (%g)", who, b, e / nu, e % nu, u[b * row + e]); return MLD_ERR_INVALID;
        }
    }
    /* staged beside the resident selection and swapped in once everything has arrived: a call that fails changes nothing */
    const hipStream_t sq = p->stream;
    mld_problem::Selection s;
    HIP_TRY(s.choice.alloc(batch)); HIP_TRY(s.policy.alloc(batch)); HIP_TRY(s.u.alloc(batch * row));
    auto stage = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(s.choice, choice, sizeof(int) * batch, hipMemcpyHostToDevice, sq));
        if (policy) HIP_TRY(hipMemcpyAsync(s.policy, policy, sizeof(int) * batch, hipMemcpyHostToDevice, sq));
        else HIP_TRY(hipMemsetAsync(s.policy, 0xff, sizeof(int) * batch, sq));      /* every byte 0xff: -1 */
        HIP_TRY(hipMemcpyAsync(s.u, u, sizeof(double) * batch * row, hipMemcpyHostToDevice, sq));
        return MLD_OK;
    };
    if (int rc = queue_and_wait(sq, stage)) return rc;
    s.K = K; s.batch = p->batch; s.has = true; s.batch_gen = p->batch_gen; s.chain = p->chain_gen;
    p->sel = std::move(s);
    return MLD_OK;
}

/* Is the kept selection the one of the current inputs?  NULL: yes; else why not (the event that ended it, as far as the two stamps tell) */
static const char *selection_stale(const mld_problem *p)
{
    if (p->sel.batch_gen != p->batch_gen) return "a batch has been uploaded since it was kept (mld_upload_batch): it belonged to the previous one";
    if (p->sel.chain != p->chain_gen) return "the inputs moved since it was kept (mld_select_inputs, mld_advance_batch, or an advancing step of any entry point): it was chosen for inputs that are gone";
    return nullptr;
}

int mld_download_selection(mld_problem_t *p, int32_t *K_out, int32_t *choice, int32_t *policy, double *u, int32_t *valid_out)
{
    static const char who[] = "mld_download_selection";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    if (!p->sel.has) { mld_set_error("%s: no kept selection (mld_keep_selection before a select call, or mld_set_selection)", who); return MLD_ERR_INVALID; }
    const mld_problem::Selection &s = p->sel;
    if (K_out) *K_out = s.K;
    if (valid_out) *valid_out = selection_stale(p) ? 0 : 1;
    if (s.batch_gen != p->batch_gen) {
        if (choice || policy || u) { mld_set_error("%s: the kept selection belonged to a batch that is gone (mld_upload_batch): only K and valid are left of it", who); return MLD_ERR_INVALID; }
        return MLD_OK;
    }
    const hipStream_t sq = p->stream;
    const size_t batch = (size_t)s.batch, len = batch * s.K * p->model->dims.nu;
    auto queue = [&]() -> int {
        if (choice) HIP_TRY(hipMemcpyAsync(choice, s.choice.get(), sizeof(int) * batch, hipMemcpyDeviceToHost, sq));
        if (policy) HIP_TRY(hipMemcpyAsync(policy, s.policy.get(), sizeof(int) * batch, hipMemcpyDeviceToHost, sq));
        if (u) HIP_TRY(hipMemcpyAsync(u, s.u.get(), sizeof(double) * len, hipMemcpyDeviceToHost, sq));
        return MLD_OK;
    };
    return queue_and_wait(sq, queue);
}

int mld_sim_step_selected(mld_problem_t *p, mld_problem_t *aux, int fb, const int64_t *act_start, int step, int flags,
                          double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out,
                          double *v0_out, int32_t *aux_status_out, int32_t *u_source_out, int32_t *n_skipped_out, int32_t *pick_out)
{
    static const char who[] = "mld_sim_step_selected";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    if (fb & ~(MLD_FB_MEMORY | MLD_FB_POLICY)) { mld_set_error("%s: unknown fallback bits 0x%x (MLD_FB_MEMORY | MLD_FB_POLICY)", who, fb); return MLD_ERR_INVALID; }
    if (p->model->dims.nu < 1) { mld_set_error("%s: the model has no input (nu = 0): there is no u a selection could supply", who); return MLD_ERR_INVALID; }
    if (!p->sel.has) { mld_set_error("%s: no kept selection (mld_keep_selection before a select call, or mld_set_selection)", who); return MLD_ERR_INVALID; }
    if (const char *why = selection_stale(p)) { mld_set_error("%s: the kept selection is stale -- %s (select again)", who, why); return MLD_ERR_INVALID; }
    if ((fb & MLD_FB_MEMORY) && !p->mem_on) { mld_set_error("%s: MLD_FB_MEMORY, but no plan memory is enabled (mld_plan_memory)", who); return MLD_ERR_INVALID; }
    if ((fb & MLD_FB_POLICY) && !p->pol_on) { mld_set_error("%s: MLD_FB_POLICY, but no policy uploaded (mld_upload_policy)", who); return MLD_ERR_INVALID; }
    if ((fb & MLD_FB_POLICY) && !p->pol_all_ruled) {
        mld_set_error("%s: MLD_FB_POLICY, but the resident policy passes a channel through (mode 0): an instance without a choice has no u such a channel could take", who);
        return MLD_ERR_INVALID;
    }
    FallbackCall fc{fb, u_source_out};
    fc.selected = true; fc.pick_out = pick_out;
    return sim_step_resolve_impl(who, false, p, aux, nullptr, act_start, step, flags, x_k1_out, y_out, cons_out, cons_vio_out, cons_row_out, v0_out, aux_status_out,
                                 n_skipped_out, &fc);
}

int mld_download_sim_log_pick(mld_problem_t *p, int first, int count, int32_t *pick)
{
    static const char who[] = "mld_download_sim_log_pick";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const mld_problem::SimLog &L = p->slog;
    if (first < 0 || count < 0 || (long long)first + count > L.count) { mld_set_error("%s: records [%d, %lld) asked for, %d logged", who, first, (long long)first + count, L.count); return MLD_ERR_INVALID; }
    if (count == 0 || !pick) return MLD_OK;
    const size_t off = (size_t)first * p->batch, len = (size_t)count * p->batch;
    if (!L.pick) { std::fill(pick, pick + len, -2); return MLD_OK; }      /* no selected step has logged: every record is another entry point's */
    const hipStream_t sq = p->stream;
    auto queue = [&]() -> int { HIP_TRY(hipMemcpyAsync(pick, L.pick.get() + off, sizeof(int) * len, hipMemcpyDeviceToHost, sq)); return MLD_OK; };
    return queue_and_wait(sq, queue);
}

} // extern "C"
