// Rule-based feedback policies of a resident batch (mld_upload_policy, mld_set_policy_state, mld_download_policy_state, mld_rollout_policy,
// mld_sim_step_policy): the reference's non-predictive baseline, DewhTheromstatController (examples/residential_mg_with_pv_and_dewhs/controllers/
// theromstat_control.py:38-64), u_k = f(x_k, u_{k-1}) stepped through sim_step_k.  The rollout and the step are the bodies of their open-loop neighbours
// (rollout_impl, sim_step_resolve_impl) with the policy switched on; kernels: k_rollout_policy, k_policy_inputs, k_policy_commit (rollout.inc).
extern "C" {

int mld_upload_policy(mld_problem_t *p, const double *sel, const double *on_at, const double *off_at, const double *u_on, const double *u_off, const int32_t *mode)
{
    static const char who[] = "mld_upload_policy";
    if (int rc = entry_guard(p, who, true, nullptr)) return rc;
    if (!p) { mld_set_error("%s: null problem", who); return MLD_ERR_INVALID; }
    if (!sel) {      /* the policy removed, and the state that belonged to it */
        p->pol_tab.reset(); p->pol_uprev.reset(); p->pol_host.clear(); p->pol_on = p->pol_all_ruled = false; p->pol_state_gen = 0;
        return MLD_OK;
    }
    const int M = p->n_models, nx = p->model->dims.nx, nu = p->model->dims.nu, row = nx + POL_TAIL;
    if (nu < 1) { mld_set_error("%s: the model has no input (nu = 0): there is nothing a policy could rule", who); return MLD_ERR_INVALID; }
    if (!on_at || !off_at || !u_on || !u_off || !mode) { mld_set_error("%s: sel given, but on_at, off_at, u_on, u_off or mode is NULL", who); return MLD_ERR_INVALID; }
    std::vector<double> tab((size_t)M * nu * row);
    bool all = true;
    if (int rc = policy_table_fill(who, -1, M, nx, nu, sel, on_at, off_at, u_on, u_off, mode, tab.data(), &all)) return rc;
    DevBuf<double> d;
    HIP_TRY(d.alloc(tab.size()));
    HIP_TRY(hipMemcpy(d, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    p->pol_tab = std::move(d); p->pol_host = std::move(tab); p->pol_on = true; p->pol_all_ruled = all;
    p->pol_uprev.reset(); p->pol_state_gen = 0;      /* the state belonged to the previous policy: reset (the new u_off) on first use */
    return MLD_OK;
}

int mld_set_policy_state(mld_problem_t *p, const double *u_prev)
{
    static const char who[] = "mld_set_policy_state";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    if (!p->pol_on) { mld_set_error("%s: no policy uploaded (mld_upload_policy)", who); return MLD_ERR_INVALID; }
    const size_t len = (size_t)p->batch * p->model->dims.nu;
    if (!u_prev) { p->pol_state_gen = 0; return policy_state_ready(p, who); }
    for (size_t k = 0; k < len; ++k) if (!std::isfinite(u_prev[k])) {
        mld_set_error("%s: u_prev of instance %zu, input %zu is not finite (%g)", who, k / p->model->dims.nu, k % p->model->dims.nu, u_prev[k]); return MLD_ERR_INVALID;
    }
    DevBuf<double> d;
    HIP_TRY(d.alloc(std::max<size_t>(1, len)));
    HIP_TRY(hipMemcpy(d, u_prev, sizeof(double) * len, hipMemcpyHostToDevice));
    p->pol_uprev = std::move(d); p->pol_state_gen = p->batch_gen;
    return MLD_OK;
}

int mld_download_policy_state(mld_problem_t *p, double *u_prev_out)
{
    static const char who[] = "mld_download_policy_state";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    if (int rc = policy_state_ready(p, who)) return rc;
    if (!u_prev_out) return MLD_OK;
    const hipStream_t sq = p->stream;
    const size_t len = (size_t)p->batch * p->model->dims.nu;
    auto queue = [&]() -> int { HIP_TRY(hipMemcpyAsync(u_prev_out, p->pol_uprev.get(), sizeof(double) * len, hipMemcpyDeviceToHost, sq)); return MLD_OK; };
    return queue_and_wait(sq, queue);
}

int mld_rollout_policy(mld_problem_t *p, mld_problem_t *aux, int K, int S, const double *u_seq, const double *u_prev, const double *omega_seq, const int64_t *start,
                       int step, const double *cost_w, int cost_rows, double *x_out, double *v_out, double *y_out, double *cons_vio_out, int32_t *cons_row_out,
                       double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out, int32_t *end_status_out,
                       int32_t *switches_out, int64_t stats[4])
{
    static const char who[] = "mld_rollout_policy";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const PolicyCall pc{u_prev, switches_out};
    const RolloutOut out{x_out, v_out, y_out, cons_vio_out, cons_row_out, cost_out, mu_total_out, worst_vio_out, worst_step_out, steps_done_out, end_status_out, stats};
    return rollout_impl(who, &pc, p, aux, K, S, u_seq, omega_seq, start, step, cost_w, cost_rows, out);
}

int mld_sim_step_policy(mld_problem_t *p, mld_problem_t *aux, const double *u0, const int64_t *act_start, int step, int flags,
                        double *x_k1_out, double *y_out, uint8_t *cons_out, double *cons_vio_out, int32_t *cons_row_out,
                        double *v0_out, int32_t *aux_status_out, int32_t *n_skipped_out)
{
    static const char who[] = "mld_sim_step_policy";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    return sim_step_resolve_impl(who, true, p, aux, u0, act_start, step, flags, x_k1_out, y_out, cons_out, cons_vio_out, cons_row_out, v0_out, aux_status_out, n_skipped_out);
}

} // extern "C"
