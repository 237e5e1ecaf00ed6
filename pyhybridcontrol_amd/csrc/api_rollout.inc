// Open-loop rollout of the resident batch's plans under realised disturbances (mld_rollout_batch, kernel k_rollout in rollout.inc).
enum { RO_MODE_ALL = MLD_ROLLOUT_COMPLETE_DEVICE | MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY };

/* The device completion's dense solve (rollout.inc: DEVICE COMPLETION): the listed slots of the resolver's resident batch, whose inputs the re-run kernel has
 * written, solved by k_solve with the small path bypassed -- what launch() does for the instances k_small_milp declined: the dense path's right-hand sides
 * and cost, the list as the work queue's order.  A MIP start, cutoffs or open-node recording of the resolver have no part in it, as after the new inputs of
 * mld_sim_step_resolve.  Host-synchronous on the resolver's stream. */
static int rollout_solve_slots(mld_problem *q, const std::vector<int> &slots)
{
    const hipStream_t sq = q->stream;
    const bool warm = q->has_warm, cut = q->has_cutoff, open = q->want_open;
    q->has_warm = q->has_cutoff = q->want_open = false;
    auto queue = [&]() -> int {
        HIP_TRY(hipMemsetAsync(q->d_counter, 0, sizeof(int), sq));
        if (int rc = launch_rhs_cost(q)) return rc;
        q->S.qp = 0;
        const ProblemDev P = problem_dev(q);
        BatchDev B = batch_dev(q, false);
        HIP_TRY(hipMemcpyAsync(q->bat.order, slots.data(), sizeof(int) * slots.size(), hipMemcpyHostToDevice, sq));
        q->order_batch = 0;
        B.order = q->bat.order; B.batch = (int)slots.size();
        if (q->lds_bytes > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q->lds_bytes));
        hipLaunchKernelGGL(k_solve, dim3(std::min(B.batch, q->n_slots)), dim3(SOL_NT), q->lds_bytes, sq, q->S, P, B, q->d_ws.get());
        HIP_TRY(hipGetLastError());
        return MLD_OK;
    };
    const int rc = queue_and_wait(sq, queue);
    q->has_warm = warm; q->has_cutoff = cut; q->want_open = open;
    return rc;
}

/* The body mld_rollout_batch and mld_rollout_policy share.  pc == nullptr: the open-loop rollout, kernel k_rollout, as it always was.  pc: the policy
 * instantiation k_rollout_policy -- the ruled channels of u_k by p's resident policy from the trajectory's own x_k and u_{k-1}, u_seq / the plan for the
 * passed-through ones only (no plan is needed when every channel is ruled), pc->u_prev (batch, nu) or the resident policy state before step 0.
 * sc (mld_warm_start_from_rollout, api_start.inc): a third way to name the disturbance -- the RESIDENT FORECAST, bat.omega (batch, N_tilde nomega), which is
 * step-major and so already the (batch, 1, K, nomega) the kernels read: K = N_tilde, S = 1, nothing uploaded or copied -- and v / end_status stay on the device:
 * k_warm_from_rollout, queued behind the rollout on the same stream, turns them into the MIP start.  The forecast is fp64 on every handle, MLD_F32 included
 * (the flag moves GEMMs to fp32, never the inputs), so the start comes from the buffers the rollout reads anyway and nothing is converted.
 * kc (mld_rollout_kpi): the KPI instantiations k_rollout_kpi / k_rollout_policy_kpi -- the column statistics of every trajectory, reduced inside the
 * kernel.  Its tables are tested as mld_sim_log_summary tests them, its price starts by the price library's window rule with len = K, the weights are laid
 * out KPI-minor as k_log_summary reads them, and everything it uploads and the kernel writes lives in temporaries of the call.
 * rk (mld_rollout_risk): the statistics ACROSS the realisations of every instance (rollout_risk.inc: THE RULE) -- the per-trajectory results the columns read
 * get their device temporaries whether or not the caller asked for them (as sc forces d_v and d_es), k_rollout_risk is queued behind the rollout kernel on
 * the same stream and its results are downloaded inside the same queue_and_wait.  The rank table idx[l][n] is built here, once per call.
 * sl (mld_rollout_select, always with rk, never with pc or sc): P candidate input sequences per instance under the same S realisations -- the kernels
 * k_rollout_cand / k_rollout_cand_kpi over batch P S trajectories, t = (b P + p) S + c, while the disturbance buffer stays (batch S, K nw), filled once as
 * for any other call; k_rollout_risk launched unchanged over batch P "instances"; k_plan_select (plan_select.inc: THE RULE) queued behind it.  The risk
 * arrays the rule reads get their device temporaries whether or not the caller asked for them; the candidates, the choice and the chosen inputs live in
 * temporaries of the call.
 * sl with sl->T > 0 (mld_rollout_select_policy): the last T candidates are rule policies in closed loop -- the kernels k_rollout_cand_policy /
 * k_rollout_cand_policy_kpi, ro_run<true> with a table per candidate (the caller's T tables and one whose every channel is passed through, for the plan and
 * the sequences), u_prev the caller's or the resident policy state; the switches source is allowed; k_plan_select writes no inputs and k_select_inputs,
 * queued behind it, writes the chosen ones.  The tables are tested by policy_table_fill, mld_upload_policy's own test, and live in a temporary. */
static int rollout_impl(const char *who, const PolicyCall *pc, mld_problem_t *p, mld_problem_t *aux, int K, int S, const double *u_seq, const double *omega_seq,
                        const int64_t *start, int step, const double *cost_w, int cost_rows, const RolloutOut &out, const StartCall *sc = nullptr,
                        const KpiCall *kc = nullptr, const RiskCall *rk = nullptr, const SelectCall *sl = nullptr)
{
    double *const x_out = out.x, *const v_out = out.v, *const y_out = out.y, *const cons_vio_out = out.cons_vio, *const cost_out = out.cost,
           *const mu_total_out = out.mu_total, *const worst_vio_out = out.worst_vio;
    int32_t *const cons_row_out = out.cons_row, *const worst_step_out = out.worst_step, *const steps_done_out = out.steps_done, *const end_status_out = out.end_status;
    int64_t *const stats = out.stats;
    mld_model *mo = p->model;
    const mld_dims &d = mo->dims;
    const int batch = p->batch, nx = d.nx, nu = d.nu, nw = d.nomega, nv = p->nv, ny = d.ny;
    if (mo->tv_N > 0) { mld_set_error("%s: time-varying models (mld_model_create_tv) are not rolled out on the device -- the step models would have to shift with the horizon", who); return MLD_ERR_INVALID; }
    if (!mo->d_pack) { mld_set_error("%s: model without matrices", who); return MLD_ERR_INVALID; }
    if (pc && !p->pol_on) { mld_set_error("%s: no policy uploaded (mld_upload_policy)", who); return MLD_ERR_INVALID; }
    if (K < 1 || S < 1) { mld_set_error("%s: K = %d, S = %d (at least one step and one realisation)", who, K, S); return MLD_ERR_INVALID; }
    if ((long long)batch * S > INT_MAX) { mld_set_error("%s: batch x S = %lld trajectories (at most %d)", who, (long long)batch * S, INT_MAX); return MLD_ERR_INVALID; }
    if (sl) {
        if (pc || sc || !rk || u_seq) { mld_set_error("%s: internal: a selection is an open-loop risk call over u_cand", who); return MLD_ERR_INVALID; }
        if (sl->P < 1 || sl->P > MLD_SELECT_P_MAX) { mld_set_error("%s: P = %d candidates (1 .. MLD_SELECT_P_MAX = %d: a lane of the wave per candidate)", who, sl->P, MLD_SELECT_P_MAX); return MLD_ERR_INVALID; }
        if ((long long)batch * S * sl->P > INT_MAX) { mld_set_error("%s: batch x P x S = %lld trajectories (at most %d)", who, (long long)batch * S * sl->P, INT_MAX); return MLD_ERR_INVALID; }
        if (sl->T < 0) { mld_set_error("%s: T = %d policy candidates (at least 0)", who, sl->T); return MLD_ERR_INVALID; }
        if (sl->T > sl->P - (sl->plan_first ? 1 : 0)) {
            mld_set_error("%s: T = %d policy candidates, but P = %d candidates in all%s (P counts the policies)", who, sl->T, sl->P, sl->plan_first ? ", the resident plan among them" : "");
            return MLD_ERR_INVALID;
        }
    }
    const int n_pol = sl ? sl->T : 0;      /* the closed-loop candidates of a selection: the last n_pol of its P */
    if (n_pol) {
        if (!(sl->pol_sel && sl->pol_on_at && sl->pol_off_at && sl->pol_u_on && sl->pol_u_off && sl->pol_mode)) {
            mld_set_error("%s: pol_sel, pol_on_at, pol_off_at, pol_u_on, pol_u_off or pol_mode is NULL with T = %d", who, n_pol); return MLD_ERR_INVALID;
        }
        if (nu < 1) { mld_set_error("%s: the model has no input (nu = 0): there is nothing a policy could rule", who); return MLD_ERR_INVALID; }
        if (!sl->u_prev && !p->pol_on) { mld_set_error("%s: u_prev is NULL, but no policy is resident (mld_upload_policy): there is no resident policy state to read", who); return MLD_ERR_INVALID; }
    }
    /* the tables of the policy candidates in the kernels' rows, and behind them one whose every channel is passed through (all zero: mode 0) */
    const size_t ptab_len = (size_t)nu * (nx + POL_TAIL), ptab_all = n_pol ? (size_t)(n_pol + 1) * p->n_models * ptab_len : 0;
    std::vector<double> hptab(ptab_all, 0.0);
    for (int t = 0; t < n_pol; ++t) {
        const size_t c = (size_t)t * p->n_models * nu;
        if (int rc = policy_table_fill(who, t, p->n_models, nx, nu, sl->pol_sel + c * nx, sl->pol_on_at + c, sl->pol_off_at + c, sl->pol_u_on + c, sl->pol_u_off + c,
                                       sl->pol_mode + c, hptab.data() + (size_t)t * p->n_models * ptab_len, nullptr)) return rc;
    }
    if (step < 0 || step > INT_MAX - K) { mld_set_error("%s: step = %d (must be >= 0)", who, step); return MLD_ERR_INVALID; }
    if (int rc = aux_fold_check(who, "rolled-out", p, aux)) return rc;
    if (aux) {
        if (!aux->small_ok) {
            mld_set_error("%s: aux is not on the small-problem path (%s): the rollout solves its auxiliary problems in LDS and has no dense fall-back -- create the resolver with MLD_SMALL_LDS, or step with mld_sim_step_resolve",
                          who, (aux->opts.flags & MLD_SMALL_LDS) ? "its shape does not fit a wave's share of LDS" : "MLD_SMALL_LDS is not set");
            return MLD_ERR_INVALID;
        }
        if (aux->has_quad || aux->ic_ld || aux->has_fixed) { mld_set_error("%s: aux has a quadratic or per-instance cost, or fixed binaries (the rollout minimises the resolver's model cost, sum(mu), with every binary free)", who); return MLD_ERR_INVALID; }
    }
    /* the KPI tables: mld_sim_log_summary's tests, where they apply */
    const int n_kpi = kc ? kc->n_kpi : 0, n_models = p->n_models, C = p->pr_chan;
    const int kw[5] = {nx, nv, ny, nw, nx};
    int k_rows = 0; unsigned k_given = 0; bool priced = false;
    if (kc) {
        static const char *const names[5] = {"w_x", "w_v", "w_y", "w_omega", "w_xk1"};
        if (n_kpi < 1 || n_kpi > MLD_KPI_MAX) { mld_set_error("%s: n_kpi = %d (1 .. MLD_KPI_MAX = %d)", who, n_kpi, MLD_KPI_MAX); return MLD_ERR_INVALID; }
        if (!kc->tab[0] && !kc->tab[1] && !kc->tab[2] && !kc->tab[3] && !kc->tab[4]) { mld_set_error("%s: w_x, w_v, w_y, w_omega and w_xk1 are all NULL: a KPI needs a table", who); return MLD_ERR_INVALID; }
        for (int t = 0; t < 5; ++t) {
            if (!kc->tab[t]) continue;
            if (kw[t] == 0) { mld_set_error("%s: %s given but the model has none of that variable (width 0)", who, names[t]); return MLD_ERR_INVALID; }
            const size_t len = (size_t)n_models * n_kpi * kw[t];
            for (size_t i = 0; i < len; ++i) if (!std::isfinite(kc->tab[t][i])) {
                mld_set_error("%s: %s of model %zu, KPI %zu, entry %zu is not finite (%g)", who, names[t], i / ((size_t)n_kpi * kw[t]), i / kw[t] % n_kpi, i % kw[t], kc->tab[t][i]);
                return MLD_ERR_INVALID;
            }
            k_given |= 1u << t; k_rows += kw[t];
        }
        if (kc->thresh) for (size_t i = 0; i < (size_t)n_models * n_kpi; ++i) if (std::isnan(kc->thresh[i])) {
            mld_set_error("%s: thresh of model %zu, KPI %zu is NaN", who, i / n_kpi, i % n_kpi); return MLD_ERR_INVALID;
        }
        if (std::isnan(kc->vio_tol)) { mld_set_error("%s: vio_tol is NaN", who); return MLD_ERR_INVALID; }
        if (kc->price_chan) for (int q = 0; q < n_kpi; ++q) {
            const int c = kc->price_chan[q];
            if (c < -1) { mld_set_error("%s: price_chan[%d] = %d (-1 = not priced, or a channel 0 .. n_chan - 1)", who, q, c); return MLD_ERR_INVALID; }
            if (c >= 0 && !p->pr_len) { mld_set_error("%s: price_chan[%d] = %d, but no price library is resident (mld_upload_prices)", who, q, c); return MLD_ERR_INVALID; }
            if (c >= C) { mld_set_error("%s: price_chan[%d] = %d, but the price library has n_chan = %d", who, q, c, C); return MLD_ERR_INVALID; }
            if (c >= 0 && !kc->price_start) { mld_set_error("%s: price_chan[%d] = %d, but price_start is NULL (the starts of the realised prices, one per instance)", who, q, c); return MLD_ERR_INVALID; }
            priced = priced || c >= 0;
        }
        if (priced) { std::vector<long long> pmax; if (int rc = check_starts(price_lib(p), who, PF_PRICE, kc->price_start, batch, 1, step, K, pmax)) return rc; }
    }
    /* the risk columns */
    unsigned r_src = 0, r_need = 0;      /* bit s: some column has source s; bit t: some column reads KPI array t of sum, min, max, n_above, n_changes */
    if (rk) {
        if (S > MLD_RISK_S_MAX) { mld_set_error("%s: S = %d realisations (at most MLD_RISK_S_MAX = %d: a lane of the wave per realisation)", who, S, MLD_RISK_S_MAX); return MLD_ERR_INVALID; }
        if (rk->G < 1 || rk->G > MLD_RISK_COLS_MAX) { mld_set_error("%s: G = %d columns (1 .. MLD_RISK_COLS_MAX = %d)", who, rk->G, MLD_RISK_COLS_MAX); return MLD_ERR_INVALID; }
        if (rk->L < 0 || rk->L > MLD_RISK_LEVELS_MAX) { mld_set_error("%s: L = %d levels (0 .. MLD_RISK_LEVELS_MAX = %d)", who, rk->L, MLD_RISK_LEVELS_MAX); return MLD_ERR_INVALID; }
        if (!rk->col_src) { mld_set_error("%s: col_src is NULL (the source of each of the G columns)", who); return MLD_ERR_INVALID; }
        if (rk->L > 0 && !rk->alpha) { mld_set_error("%s: alpha is NULL with L = %d levels", who, rk->L); return MLD_ERR_INVALID; }
        for (int j = 0; j < rk->G; ++j) {
            const int s = rk->col_src[j], q = rk->col_q ? rk->col_q[j] : 0;
            if (s < 0 || s >= RISK_N_SRC) { mld_set_error("%s: col_src[%d] = %d (a source 0 .. %d)", who, j, s, RISK_N_SRC - 1); return MLD_ERR_INVALID; }
            if (s == RISK_SWITCHES && !pc && !n_pol) { mld_set_error("%s: col_src[%d] = %d (switches), but the rollout has no policy (policy == 0)", who, j, s); return MLD_ERR_INVALID; }
            if (s >= RISK_N_VIO && n_kpi == 0) { mld_set_error("%s: col_src[%d] = %d reads the KPIs, but n_kpi = 0 (no KPI table in this call)", who, j, s); return MLD_ERR_INVALID; }
            if (s >= RISK_KPI_SUM && (q < 0 || q >= n_kpi)) { mld_set_error("%s: col_q[%d] = %d (a KPI 0 .. n_kpi - 1 = %d)", who, j, q, n_kpi - 1); return MLD_ERR_INVALID; }
            if (rk->level && std::isnan(rk->level[j])) { mld_set_error("%s: level[%d] is NaN", who, j); return MLD_ERR_INVALID; }
            r_src |= 1u << s;
            if (s >= RISK_KPI_SUM) r_need |= 1u << (s - RISK_KPI_SUM);
        }
        for (int l = 0; l < rk->L; ++l) if (!(rk->alpha[l] > 0.0 && rk->alpha[l] <= 1.0)) {
            mld_set_error("%s: alpha[%d] = %g (a level in (0, 1])", who, l, rk->alpha[l]); return MLD_ERR_INVALID;
        }
    }
    /* the selection rule */
    const int n_own = sl ? sl->P - (sl->plan_first ? 1 : 0) - n_pol : 0;      /* candidates of u_cand */
    unsigned s_kinds = 0;                                            /* bit k: some statistic of the rule has kind k */
    if (sl) {
        auto stat_ok = [&](const char *col_name, const char *kind_name, const char *lvl_name, int k, int col, int kind, int lvl) -> bool {
            char at[16] = "";
            if (k >= 0) snprintf(at, sizeof at, "[%d]", k);
            if (col < 0 || col >= rk->G) { mld_set_error("%s: %s%s = %d (a column 0 .. G - 1 = %d)", who, col_name, at, col, rk->G - 1); return false; }
            if (kind < 0 || kind >= SEL_N_KIND) { mld_set_error("%s: %s%s = %d (a kind 0 .. %d: mean, min, max, n_exceed, quantile, cvar_hi, cvar_lo)", who, kind_name, at, kind, SEL_N_KIND - 1); return false; }
            if (kind >= SEL_QUANTILE && (lvl < 0 || lvl >= rk->L)) { mld_set_error("%s: %s%s = %d (a level index 0 .. L - 1 = %d; kind %d is per level)", who, lvl_name, at, lvl, rk->L - 1, kind); return false; }
            s_kinds |= 1u << kind;
            return true;
        };
        if (n_own > 0 && !sl->u_cand) { mld_set_error("%s: u_cand is NULL (the %d candidate sequences per instance%s)", who, n_own, sl->plan_first ? " beside the resident plan" : ""); return MLD_ERR_INVALID; }
        if (!stat_ok("obj_col", "obj_kind", "obj_level", -1, sl->obj_col, sl->obj_kind, sl->obj_level)) return MLD_ERR_INVALID;
        if (sl->n_cons < 0 || sl->n_cons > MLD_SELECT_CONS_MAX) { mld_set_error("%s: n_cons = %d constraints (0 .. MLD_SELECT_CONS_MAX = %d)", who, sl->n_cons, MLD_SELECT_CONS_MAX); return MLD_ERR_INVALID; }
        if (sl->n_cons > 0 && !(sl->cons_col && sl->cons_kind && sl->cons_bound)) { mld_set_error("%s: cons_col, cons_kind or cons_bound is NULL with n_cons = %d", who, sl->n_cons); return MLD_ERR_INVALID; }
        for (int k = 0; k < sl->n_cons; ++k) {
            if (!stat_ok("cons_col", "cons_kind", "cons_level", k, sl->cons_col[k], sl->cons_kind[k], sl->cons_level ? sl->cons_level[k] : 0)) return MLD_ERR_INVALID;
            if (std::isnan(sl->cons_bound[k])) { mld_set_error("%s: cons_bound[%d] is NaN", who, k); return MLD_ERR_INVALID; }
        }
        if (sl->min_complete < 1 || sl->min_complete > S) { mld_set_error("%s: min_complete = %d (1 .. S = %d)", who, sl->min_complete, S); return MLD_ERR_INVALID; }
    }
    const size_t stage_d = ro_stage_doubles(nx, nu, nw, aux ? aux->m0 : 0, nv, ny, n_kpi);
    if (sizeof(double) * stage_d > SM_WAVE_BUDGET) {
        mld_set_error("%s: the staging of a trajectory (%zu bytes: x, omega', h, v, y, x_k1) does not fit a wave's share of LDS (%d bytes); step with mld_sim_step_resolve", who, sizeof(double) * stage_d, SM_WAVE_BUDGET);
        return MLD_ERR_INVALID;
    }
    const bool by_plan = sl ? sl->plan_first != 0 : (!u_seq && !(pc && p->pol_all_ruled));      /* some channel takes the resident plan's input */
    if (by_plan) {      /* the plan-state tests of sim_step_check */
        if (K > p->N) { mld_set_error("%s: K = %d steps with the resident plan's inputs, but the plan has N_tilde = %d (pass u_seq for a longer rollout)", who, K, p->N); return MLD_ERR_INVALID; }
        if (!p->solved) { mld_set_error("%s: the resident batch has not been solved since its upload / selection (there is no plan to apply; pass u_seq)", who); return MLD_ERR_INVALID; }
        if (p->advanced) { mld_set_error("%s: the last solve's plan has already been applied -- the resident plan belongs to inputs that are gone (solve again, or pass u_seq)", who); return MLD_ERR_INVALID; }
    }
    if (sc) {
        if (K != p->N || S != 1 || omega_seq || start || (size_t)K * nw != (size_t)p->nW) { mld_set_error("%s: internal: the resident forecast is (batch, N_tilde, nomega)", who); return MLD_ERR_INVALID; }
    } else if (nw) {
        if ((omega_seq != nullptr) == (start != nullptr)) { mld_set_error("%s: exactly one of omega_seq and start must be given (%s)", who, omega_seq ? "both are" : "neither is"); return MLD_ERR_INVALID; }
    } else if (start) { mld_set_error("%s: start given, but the model has no disturbance (nomega = 0)", who); return MLD_ERR_INVALID; }
    if (cost_w && cost_rows != p->n_models && cost_rows != batch) { mld_set_error("%s: cost_rows = %d (n_models = %d or batch = %d)", who, cost_rows, p->n_models, batch); return MLD_ERR_INVALID; }
    std::vector<long long> gmax;
    if (start) {
        if (!p->pf_len) { mld_set_error("%s: start given, but no profile library is resident (mld_upload_profiles)", who); return MLD_ERR_INVALID; }
        if (int rc = profile_check_starts(p, who, PF_WINDOW, start, batch, S, step, K, gmax)) return rc;
    }
    const size_t TW = (size_t)batch * S, T = TW * (size_t)(sl ? sl->P : 1);      /* the rows of the disturbance buffer, and the trajectories */
    if (sl) for (size_t k = 0; k < (size_t)batch * n_own * K * nu; ++k) if (!std::isfinite(sl->u_cand[k])) {
        mld_set_error("%s: u_cand of instance %zu, candidate %zu, step %zu, input %zu is not finite (%g)", who, k / ((size_t)n_own * K * nu), k / ((size_t)K * nu) % n_own, k / nu % K, k % nu, sl->u_cand[k]);
        return MLD_ERR_INVALID;
    }
    if (u_seq) for (size_t k = 0; k < (size_t)batch * K * nu; ++k) if (!std::isfinite(u_seq[k])) {
        mld_set_error("%s: u_seq of instance %zu, step %zu, input %zu is not finite (%g)", who, k / ((size_t)K * nu), k / nu % K, k % nu, u_seq[k]); return MLD_ERR_INVALID;
    }
    if (omega_seq && nw) for (size_t k = 0; k < TW * K * nw; ++k) if (!std::isfinite(omega_seq[k])) {
        mld_set_error("%s: omega_seq of trajectory %zu, step %zu, channel %zu is not finite (%g)", who, k / ((size_t)K * nw), k / nw % K, k % nw, omega_seq[k]); return MLD_ERR_INVALID;
    }
    const double *const u_prev_in = pc ? pc->u_prev : (n_pol ? sl->u_prev : nullptr);      /* the caller's inputs before step 0; nullptr: the resident policy state, or no policy */
    if (u_prev_in) for (size_t k = 0; k < (size_t)batch * nu; ++k) if (!std::isfinite(u_prev_in[k])) {
        mld_set_error("%s: u_prev of instance %zu, input %zu is not finite (%g)", who, k / nu, k % nu, u_prev_in[k]); return MLD_ERR_INVALID;
    }
    const bool cw_inst = cost_w && cost_rows != p->n_models;      /* (batch == n_models: a row per model) */
    if (cost_w) for (size_t k = 0; k < (size_t)cost_rows * K * nv; ++k) if (!std::isfinite(cost_w[k])) {
        mld_set_error("%s: cost_w of row %zu, step %zu, entry %zu is not finite (%g)", who, k / ((size_t)K * nv), k / nv % K, k % nv, cost_w[k]); return MLD_ERR_INVALID;
    }

    if (sc && p->nb == 0) return MLD_OK;      /* every check has passed; without a binary there is no start to set, and nothing is rolled out */

    SmShape SS{};
    size_t wave_d = 0;
    if (aux) {
        SS = aux->SS;
        SS.max_nodes = aux->opts.max_nodes; SS.gap_abs = aux->opts.gap_abs; SS.gap_rel = aux->opts.gap_rel;
        SS.max_pivots = (aux->opts.reserved & MLD_DBG_SMALL_PIVOT_CAP) ? 2 : aux->opts.max_pivots;
        wave_d = (size_t)SS.wave_doubles;
    }
    const size_t lds_bytes = sizeof(double) * (wave_d + stage_d) * SM_WAVES;
    const hipStream_t sq = p->stream;
    const size_t Kz = (size_t)K;
    DevBuf<double> d_u, d_om, d_cw, d_x, d_v, d_y, d_vio, d_cost, d_mu, d_wv, d_uprev; DevBuf<int> d_row, d_ws, d_sd, d_es, d_sw; DevBuf<long long> d_start; DevBuf<unsigned long long> d_cnt;
    DevBuf<double> d_kW, d_kthr, d_ksum, d_kmin, d_kmax; DevBuf<int> d_kpc, d_kmins, d_kmaxs, d_kabove, d_kchg, d_knvio; DevBuf<long long> d_kps;      /* kc */
    std::vector<double> hW, hthr; std::vector<int> hpc;
    DevBuf<double> d_rlev, d_rmean, d_rmin, d_rmax, d_rq, d_rhi, d_rlo; DevBuf<int> d_rsrc, d_rcq, d_ridx, d_rminc, d_rmaxc, d_rex, d_rqc, d_rcnt;      /* rk */
    std::vector<int> hrq, hidx;
    DevBuf<double> d_ucand, d_sscore, d_such, d_su0; DevBuf<int> d_schoice, d_snadm; DevBuf<unsigned char> d_sadm;      /* sl */
    DevBuf<unsigned char> d_old; DevBuf<int> d_src;      /* sc: the resident start as it was (where rows are kept), the source per instance */
    DevBuf<double> d_ptab;      /* sl with policies: the tables */
    if ((pc || n_pol) && !u_prev_in) { if (int rc = policy_state_ready(p, who)) return rc; }      /* (an upload's reset state, laid out on first use: nothing a caller can see changes) */
    if (u_prev_in) HIP_TRY(d_uprev.alloc(std::max<size_t>(1, (size_t)batch * nu)));
    if (n_pol) HIP_TRY(d_ptab.alloc(ptab_all));
    if (u_seq) HIP_TRY(d_u.alloc(std::max<size_t>(1, (size_t)batch * Kz * nu)));
    if (!sc) HIP_TRY(d_om.alloc(std::max<size_t>(1, TW * Kz * nw)));
    if (start) HIP_TRY(d_start.alloc(TW * p->pf_groups));
    if (cost_w) HIP_TRY(d_cw.alloc(std::max<size_t>(1, (size_t)cost_rows * Kz * nv)));
    /* an output that was asked for and is not empty gets a device buffer (take), and is copied back after the kernel (get) */
    const size_t cx = T * (Kz + 1) * nx, cv = T * Kz * nv, cy = T * Kz * ny, ck = T * Kz;
    auto take = [](auto &buf, const void *out, size_t count) -> hipError_t { return out && count ? buf.alloc(count) : hipSuccess; };
    HIP_TRY(take(d_x, x_out, cx)); HIP_TRY(take(d_v, v_out, cv)); HIP_TRY(take(d_y, y_out, cy)); HIP_TRY(take(d_vio, cons_vio_out, ck)); HIP_TRY(take(d_row, cons_row_out, ck));
    HIP_TRY(take(d_cost, cost_out, T)); HIP_TRY(take(d_mu, mu_total_out, T)); HIP_TRY(take(d_wv, worst_vio_out, T));
    HIP_TRY(take(d_ws, worst_step_out, T)); HIP_TRY(take(d_sd, steps_done_out, T)); HIP_TRY(take(d_es, end_status_out, T));
    if (pc) HIP_TRY(take(d_sw, pc->switches_out, T));
    if (n_pol) HIP_TRY(take(d_sw, sl->switches_out, T));
    const bool dev_complete = (p->ro_mode & MLD_ROLLOUT_COMPLETE_DEVICE) && aux;      /* declined trajectories are finished on the device: k_ro_collect reads the endings */
    if (dev_complete && !d_es) HIP_TRY(d_es.alloc(T));
    const size_t r_inst = (size_t)batch * (size_t)(sl ? sl->P : 1);      /* what k_rollout_risk takes for its instances: i = b P + p */
    const size_t rg = rk ? r_inst * rk->G : 0, rgl = rk ? rg * rk->L : 0;
    if (rk) {      /* the temporaries of the sources the columns read, asked for or not; the rank table; the results' buffers */
        auto force = [](auto &buf, bool read, size_t count) -> hipError_t { return read && !buf ? buf.alloc(count) : hipSuccess; };
        HIP_TRY(force(d_es, true, T)); HIP_TRY(force(d_cost, r_src >> RISK_COST & 1u, T)); HIP_TRY(force(d_mu, r_src >> RISK_MU_TOTAL & 1u, T));
        HIP_TRY(force(d_wv, r_src >> RISK_WORST_VIO & 1u, T)); HIP_TRY(force(d_sw, r_src >> RISK_SWITCHES & 1u, T));
        hrq.assign(rk->G, 0);
        if (rk->col_q) std::copy(rk->col_q, rk->col_q + rk->G, hrq.begin());
        hidx.resize(std::max<size_t>(1, (size_t)rk->L * S));
        for (int l = 0; l < rk->L; ++l) for (int n = 1; n <= S; ++n) hidx[(size_t)l * S + n - 1] = risk_rank(rk->alpha[l], n);
        HIP_TRY(d_rsrc.alloc(rk->G)); HIP_TRY(d_rcq.alloc(rk->G)); HIP_TRY(d_ridx.alloc(hidx.size()));
        if (rk->level) HIP_TRY(d_rlev.alloc(rk->G));
        HIP_TRY(take(d_rmean, rk->mean, rg)); HIP_TRY(take(d_rmin, rk->min, rg)); HIP_TRY(take(d_rmax, rk->max, rg)); HIP_TRY(take(d_rminc, rk->min_c, rg));
        HIP_TRY(take(d_rmaxc, rk->max_c, rg)); HIP_TRY(take(d_rex, rk->n_exceed, rg)); HIP_TRY(take(d_rq, rk->quantile, rgl)); HIP_TRY(take(d_rqc, rk->quantile_c, rgl));
        HIP_TRY(take(d_rhi, rk->cvar_hi, rgl)); HIP_TRY(take(d_rlo, rk->cvar_lo, rgl)); HIP_TRY(take(d_rcnt, rk->counts, r_inst * 4));
    }
    const size_t s_own = (size_t)batch * n_own * Kz * nu, s_seq = (size_t)batch * Kz * nu;
    if (sl) {      /* the risk arrays the rule reads, asked for or not; the candidates; the choice */
        auto force = [](auto &buf, bool read, size_t count) -> hipError_t { return read && !buf ? buf.alloc(std::max<size_t>(1, count)) : hipSuccess; };
        HIP_TRY(force(d_rmean, s_kinds >> SEL_MEAN & 1u, rg)); HIP_TRY(force(d_rmin, s_kinds >> SEL_MIN & 1u, rg)); HIP_TRY(force(d_rmax, s_kinds >> SEL_MAX & 1u, rg));
        HIP_TRY(force(d_rex, s_kinds >> SEL_N_EXCEED & 1u, rg)); HIP_TRY(force(d_rq, s_kinds >> SEL_QUANTILE & 1u, rgl));
        HIP_TRY(force(d_rhi, s_kinds >> SEL_CVAR_HI & 1u, rgl)); HIP_TRY(force(d_rlo, s_kinds >> SEL_CVAR_LO & 1u, rgl)); HIP_TRY(force(d_rcnt, true, r_inst * 4));
        HIP_TRY(d_ucand.alloc(std::max<size_t>(1, s_own)));
        HIP_TRY(take(d_schoice, sl->choice, (size_t)batch)); HIP_TRY(take(d_sscore, sl->score, (size_t)batch)); HIP_TRY(take(d_snadm, sl->n_admissible, (size_t)batch));
        HIP_TRY(take(d_sadm, sl->admissible, r_inst)); HIP_TRY(take(d_such, sl->u_choice, s_seq)); HIP_TRY(take(d_su0, sl->u0_choice, (size_t)batch * nu));
        HIP_TRY(force(d_schoice, n_pol && (d_such || d_su0), (size_t)batch));      /* k_select_inputs reads the choice */
    }
    /* keep_selection (mld_keep_selection): the choice and the chosen inputs also stay on the device, in buffers built beside the kept ones and swapped in when
     * the call has succeeded.  Off: nothing is allocated and no copy is queued */
    const bool keep_sel = sl && p->sel_keep;
    mld_problem::Selection kept;
    if (keep_sel) {
        auto force = [](auto &buf, size_t count) -> hipError_t { return !buf ? buf.alloc(std::max<size_t>(1, count)) : hipSuccess; };
        HIP_TRY(force(d_schoice, (size_t)batch)); HIP_TRY(force(d_such, s_seq));
        HIP_TRY(kept.choice.alloc((size_t)batch)); HIP_TRY(kept.policy.alloc((size_t)batch)); HIP_TRY(kept.u.alloc(std::max<size_t>(1, s_seq)));
    }
    const size_t warm_len = sc ? (size_t)batch * p->nb : 0;
    const bool keep_rows = sc && sc->keep && p->has_warm;
    std::vector<int32_t> src_host;
    if (sc) {
        HIP_TRY(d_v.alloc(cv)); HIP_TRY(d_es.alloc(T)); HIP_TRY(d_src.alloc((size_t)batch));
        if (keep_rows) HIP_TRY(d_old.alloc(warm_len));
        src_host.resize((size_t)batch);
    }
    const size_t tq = T * (size_t)n_kpi, mq = (size_t)n_models * n_kpi;
    if (kc) {      /* the tables side by side, KPI-minor: W[m, row, q] (mld_sim_log_summary's layout) */
        hW.resize((size_t)n_models * k_rows * n_kpi); hthr.assign(mq, std::numeric_limits<double>::infinity()); hpc.assign(n_kpi, -1);
        for (int m = 0; m < n_models; ++m) {
            int row = 0;
            for (int t = 0; t < 5; ++t) {
                if (!kc->tab[t]) continue;
                for (int q = 0; q < n_kpi; ++q)
                    for (int i = 0; i < kw[t]; ++i) hW[((size_t)m * k_rows + row + i) * n_kpi + q] = kc->tab[t][((size_t)m * n_kpi + q) * kw[t] + i];
                row += kw[t];
            }
        }
        if (kc->thresh) std::copy(kc->thresh, kc->thresh + mq, hthr.begin());
        if (kc->price_chan) std::copy(kc->price_chan, kc->price_chan + n_kpi, hpc.begin());
        HIP_TRY(d_kW.alloc(hW.size())); HIP_TRY(d_kthr.alloc(mq)); HIP_TRY(d_kpc.alloc(n_kpi));
        if (priced) HIP_TRY(d_kps.alloc(batch));
        HIP_TRY(d_ksum.alloc(tq)); HIP_TRY(d_kmin.alloc(tq)); HIP_TRY(d_kmax.alloc(tq)); HIP_TRY(d_kmins.alloc(tq)); HIP_TRY(d_kmaxs.alloc(tq));
        HIP_TRY(d_kabove.alloc(tq)); HIP_TRY(d_kchg.alloc(tq)); HIP_TRY(d_knvio.alloc(T));
    }
    HIP_TRY(d_cnt.alloc(4));
    RoDev a{};
    a.batch = batch; a.S = S; a.K = K;
    a.nx = nx; a.nu = nu; a.nw = nw; a.nv = nv; a.nmu = d.nmu; a.ny = ny; a.nc = d.nc; a.m = aux ? aux->m0 : 0; a.n = aux ? aux->n : 0;
    a.stage_doubles = (int)stage_d;
    a.pack = mo->d_pack; a.pack_len = mo->pack_len; a.off = mo->pack_off;
    a.model_idx = p->has_midx ? p->bat.model_idx.get() : nullptr;
    a.x0 = p->bat.x0;
    if (u_seq) { a.u = d_u; a.u_stride = Kz * nu; a.u_step = (size_t)nu; }
    else if (sl && !by_plan) { a.u = d_ucand; a.u_stride = 0; a.u_step = 0; }      /* every candidate reads u_cand (RoCandDev) */
    else if (by_plan) { a.u = p->bat.v; a.u_stride = (size_t)p->n; a.u_step = (size_t)nv; a.status = p->bat.status; a.obj = p->bat.obj; }      /* rows < batch are the instances' (after the hand-off's device merge) */
    else { a.u = p->bat.x0; a.u_stride = 0; a.u_step = 0; }      /* every channel ruled: u is never read (a valid address all the same) */
    a.om = sc ? p->bat.omega.get() : d_om.get();
    a.cw = cost_w ? d_cw.get() : nullptr; a.cw_by_inst = cw_inst ? 1 : 0;
    a.x = d_x; a.v = d_v; a.y = d_y; a.vio = d_vio; a.row = d_row;
    a.cost = d_cost; a.mu_total = d_mu; a.worst_vio = d_wv; a.worst_step = d_ws; a.steps_done = d_sd; a.end_status = d_es;
    a.counter = d_cnt;
    ProblemDev P{};
    if (aux) P = problem_dev(aux);
    RoPolicyDev pd{};
    if (pc) { pd.tab = p->pol_tab; pd.tab_len = (size_t)nu * (nx + POL_TAIL); pd.u_prev = pc->u_prev ? d_uprev.get() : p->pol_uprev.get(); pd.switches = d_sw; }
    RoKpiDev kd{};
    if (kc) {
        kd.n_kpi = n_kpi; kd.rows = k_rows; kd.n_chan = C; kd.step = step; kd.given = k_given; kd.vio_tol = kc->vio_tol;
        kd.W = d_kW; kd.thresh = d_kthr; kd.price_chan = d_kpc;
        if (priced) { kd.lib = p->pr_lib; kd.price_start = d_kps; }
        kd.sum = d_ksum; kd.min = d_kmin; kd.max = d_kmax; kd.min_step = d_kmins; kd.max_step = d_kmaxs; kd.n_above = d_kabove; kd.n_changes = d_kchg; kd.n_vio = d_knvio;
    }
    RoCandDev cd{};
    if (sl) { cd.P = sl->P; cd.plan_first = sl->plan_first ? 1 : 0; cd.u_cand = d_ucand; }
    RoCandPolDev cq{};
    if (n_pol) {      /* of pd the candidate-policy kernels read u_prev and switches; the tables are cq's */
        pd.u_prev = u_prev_in ? d_uprev.get() : p->pol_uprev.get(); pd.switches = d_sw;
        cq.tab = d_ptab; cq.tab_len = ptab_len; cq.n_models = p->n_models; cq.n_seq = sl->P - n_pol;
    }
    const void *kernel = n_pol ? (kc ? (const void *)k_rollout_cand_policy_kpi : (const void *)k_rollout_cand_policy) : sl ? (kc ? (const void *)k_rollout_cand_kpi : (const void *)k_rollout_cand) : kc ? (pc ? (const void *)k_rollout_policy_kpi : (const void *)k_rollout_kpi) : (pc ? (const void *)k_rollout_policy : (const void *)k_rollout);
    if (lds_bytes > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    int dev = 0, per_cu = 0; hipDeviceProp_t prop;
    (void)hipGetDevice(&dev); HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, SM_NT, lds_bytes) != hipSuccess || per_cu < 1) per_cu = 1;
    const int grid = (int)std::min<size_t>((T + SM_WAVES - 1) / SM_WAVES, (size_t)per_cu * prop.multiProcessorCount);
    RiskArgs ra{};
    size_t risk_lds = 0; int risk_grid = 1;
    if (rk) {
        ra.batch = (int)r_inst; ra.S = S; ra.G = rk->G; ra.L = rk->L; ra.n_kpi = n_kpi; ra.need = r_need;
        const size_t stg = risk_stage_doubles(S, n_kpi, r_need, ra.off);
        ra.staged = r_need && sizeof(double) * RISK_WAVES * (RISK_SORT_DOUBLES + stg) <= RISK_LDS_MAX;      /* blocks that do not fit are read in place: the same bits */
        ra.ld = ra.staged ? (n_kpi | 1) : n_kpi;
        ra.wave_doubles = (int)(RISK_SORT_DOUBLES + (ra.staged ? stg : 0));
        ra.col_src = d_rsrc; ra.col_q = d_rcq; ra.level = rk->level ? d_rlev.get() : nullptr; ra.idx = d_ridx;
        ra.es = d_es; ra.cost = d_cost; ra.mu = d_mu; ra.wv = d_wv; ra.sw = d_sw; ra.nvio = d_knvio;
        ra.ksum = d_ksum; ra.kmin = d_kmin; ra.kmax = d_kmax; ra.kabove = d_kabove; ra.kchg = d_kchg;
        ra.mean = d_rmean; ra.min = d_rmin; ra.max = d_rmax; ra.min_c = d_rminc; ra.max_c = d_rmaxc; ra.n_exceed = d_rex;
        ra.quantile = d_rq; ra.quantile_c = d_rqc; ra.cvar_hi = d_rhi; ra.cvar_lo = d_rlo; ra.counts = d_rcnt;
        risk_lds = sizeof(double) * RISK_WAVES * (size_t)ra.wave_doubles;
        if (risk_lds > 48 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void *)k_rollout_risk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)risk_lds));
        int rper = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&rper, (const void *)k_rollout_risk, 64 * RISK_WAVES, risk_lds) != hipSuccess || rper < 1) rper = 1;
        risk_grid = (int)std::min<long long>(((long long)r_inst + RISK_WAVES - 1) / RISK_WAVES, (long long)rper * prop.multiProcessorCount);
    }
    SelArgs sa{};
    SelInputsArgs si{};
    int sel_grid = 1;
    if (sl) {
        sa.batch = batch; sa.P = sl->P; sa.G = rk->G; sa.L = rk->L; sa.K = K; sa.nu = nu; sa.plan_first = sl->plan_first ? 1 : 0;
        sa.rule.obj = SelStat{sl->obj_col, sl->obj_kind, sl->obj_kind >= SEL_QUANTILE ? sl->obj_level : 0};
        sa.rule.n_cons = sl->n_cons; sa.rule.min_complete = sl->min_complete;
        for (int k = 0; k < sl->n_cons; ++k) {
            sa.rule.cons[k] = SelStat{sl->cons_col[k], sl->cons_kind[k], sl->cons_kind[k] >= SEL_QUANTILE && sl->cons_level ? sl->cons_level[k] : 0};
            sa.rule.bound[k] = sl->cons_bound[k];
        }
        sa.mean = d_rmean; sa.min = d_rmin; sa.max = d_rmax; sa.n_exceed = d_rex; sa.quantile = d_rq; sa.cvar_hi = d_rhi; sa.cvar_lo = d_rlo; sa.counts = d_rcnt;
        sa.plan = p->bat.v; sa.plan_stride = (size_t)p->n; sa.plan_step = (size_t)nv; sa.u_cand = d_ucand;
        sa.choice = d_schoice; sa.score = d_sscore; sa.n_adm = d_snadm; sa.adm = d_sadm; sa.u_choice = d_such; sa.u0_choice = d_su0;
        if (n_pol) {      /* k_plan_select would index u_cand out of range for a policy pick: the chosen inputs are k_select_inputs', behind it */
            sa.u_choice = sa.u0_choice = nullptr;
            si.batch = batch; si.P = sl->P; si.K = K; si.nu = nu; si.nx = nx; si.plan_first = sa.plan_first; si.n_seq = sl->P - n_pol; si.n_models = p->n_models;
            si.choice = d_schoice; si.plan = sa.plan; si.plan_stride = sa.plan_stride; si.plan_step = sa.plan_step; si.u_cand = d_ucand;
            si.tab = d_ptab; si.tab_len = ptab_len; si.model_idx = a.model_idx; si.x0 = p->bat.x0; si.u_prev = pd.u_prev;
            si.u_choice = d_such; si.u0_choice = d_su0;
        }
        int sper = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&sper, (const void *)k_plan_select, 64 * SEL_WAVES, 0) != hipSuccess || sper < 1) sper = 1;
        sel_grid = (int)std::min<long long>(((long long)batch + SEL_WAVES - 1) / SEL_WAVES, (long long)sper * prop.multiProcessorCount);
    }
    unsigned long long cnt[4] = {};
    /* everything queued on the stream and waited for on every path (queue_and_wait): the caller's arrays and the temporaries may go when this returns */
    auto queue_rollout = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(cnt), sq));
        if (u_seq && nu) HIP_TRY(hipMemcpyAsync(d_u, u_seq, sizeof(double) * (size_t)batch * Kz * nu, hipMemcpyHostToDevice, sq));
        if (u_prev_in && nu) HIP_TRY(hipMemcpyAsync(d_uprev, u_prev_in, sizeof(double) * (size_t)batch * nu, hipMemcpyHostToDevice, sq));
        if (n_pol) HIP_TRY(hipMemcpyAsync(d_ptab, hptab.data(), sizeof(double) * ptab_all, hipMemcpyHostToDevice, sq));
        if (cost_w && nv) HIP_TRY(hipMemcpyAsync(d_cw, cost_w, sizeof(double) * (size_t)cost_rows * Kz * nv, hipMemcpyHostToDevice, sq));
        if (sl && s_own) HIP_TRY(hipMemcpyAsync(d_ucand, sl->u_cand, sizeof(double) * s_own, hipMemcpyHostToDevice, sq));
        if (omega_seq && nw) HIP_TRY(hipMemcpyAsync(d_om, omega_seq, sizeof(double) * TW * Kz * nw, hipMemcpyHostToDevice, sq));
        if (start) {      /* the windows of K steps gathered into the buffer omega_seq would be uploaded to: one input layout for the kernel */
            HIP_TRY(hipMemcpyAsync(d_start, start, sizeof(long long) * TW * p->pf_groups, hipMemcpyHostToDevice, sq));
            hipLaunchKernelGGL(k_profile_windows, dim3(profile_grid((long long)TW * K * nw)), dim3(256), 0, sq, (int)TW, K * nw, nw, S, S, 0, p->pf_groups, d_start.get(),
                               p->pf_chan.get(), step, p->pf_lib.get(), d_om.get());
            HIP_TRY(hipGetLastError());
        }
        if (kc) {
            HIP_TRY(hipMemcpyAsync(d_kW, hW.data(), sizeof(double) * hW.size(), hipMemcpyHostToDevice, sq));
            HIP_TRY(hipMemcpyAsync(d_kthr, hthr.data(), sizeof(double) * mq, hipMemcpyHostToDevice, sq));
            HIP_TRY(hipMemcpyAsync(d_kpc, hpc.data(), sizeof(int) * n_kpi, hipMemcpyHostToDevice, sq));
            if (priced) HIP_TRY(hipMemcpyAsync(d_kps, kc->price_start, sizeof(long long) * (size_t)batch, hipMemcpyHostToDevice, sq));
        }
        if (rk) {
            HIP_TRY(hipMemcpyAsync(d_rsrc, rk->col_src, sizeof(int) * (size_t)rk->G, hipMemcpyHostToDevice, sq));
            HIP_TRY(hipMemcpyAsync(d_rcq, hrq.data(), sizeof(int) * (size_t)rk->G, hipMemcpyHostToDevice, sq));
            HIP_TRY(hipMemcpyAsync(d_ridx, hidx.data(), sizeof(int) * hidx.size(), hipMemcpyHostToDevice, sq));
            if (rk->level) HIP_TRY(hipMemcpyAsync(d_rlev, rk->level, sizeof(double) * (size_t)rk->G, hipMemcpyHostToDevice, sq));
        }
        if (n_pol && kc) hipLaunchKernelGGL(k_rollout_cand_policy_kpi, dim3(grid), dim3(SM_NT), lds_bytes, sq, SS, P, a, cd, pd, cq, kd);
        else if (n_pol) hipLaunchKernelGGL(k_rollout_cand_policy, dim3(grid), dim3(SM_NT), lds_bytes, sq, SS, P, a, cd, pd, cq);
        else if (sl && kc) hipLaunchKernelGGL(k_rollout_cand_kpi, dim3(grid), dim3(SM_NT), lds_bytes, sq, SS, P, a, cd, kd);
        else if (sl) hipLaunchKernelGGL(k_rollout_cand, dim3(grid), dim3(SM_NT), lds_bytes, sq, SS, P, a, cd);
        else if (kc && pc) hipLaunchKernelGGL(k_rollout_policy_kpi, dim3(grid), dim3(SM_NT), lds_bytes, sq, SS, P, a, pd, kd);
        else if (kc) hipLaunchKernelGGL(k_rollout_kpi, dim3(grid), dim3(SM_NT), lds_bytes, sq, SS, P, a, kd);
        else if (pc) hipLaunchKernelGGL(k_rollout_policy, dim3(grid), dim3(SM_NT), lds_bytes, sq, SS, P, a, pd);
        else hipLaunchKernelGGL(k_rollout, dim3(grid), dim3(SM_NT), lds_bytes, sq, SS, P, a);
        HIP_TRY(hipGetLastError());
        return MLD_OK;
    };
    /* what reads the trajectories' results: queued behind the rollout kernel, or behind the device completion where that is on */
    auto queue_readers = [&]() -> int {
        auto get = [&](auto *out, const auto &buf, size_t count) -> hipError_t {
            return out && buf ? hipMemcpyAsync(out, buf, sizeof(*out) * count, hipMemcpyDeviceToHost, sq) : hipSuccess;
        };
        if (rk) {      /* behind the rollout kernel on the same stream: its per-trajectory results are this kernel's input */
            hipLaunchKernelGGL(k_rollout_risk, dim3(risk_grid), dim3(64 * RISK_WAVES), risk_lds, sq, ra);
            HIP_TRY(hipGetLastError());
            HIP_TRY(get(rk->mean, d_rmean, rg)); HIP_TRY(get(rk->min, d_rmin, rg)); HIP_TRY(get(rk->max, d_rmax, rg)); HIP_TRY(get(rk->min_c, d_rminc, rg));
            HIP_TRY(get(rk->max_c, d_rmaxc, rg)); HIP_TRY(get(rk->n_exceed, d_rex, rg)); HIP_TRY(get(rk->quantile, d_rq, rgl)); HIP_TRY(get(rk->quantile_c, d_rqc, rgl));
            HIP_TRY(get(rk->cvar_hi, d_rhi, rgl)); HIP_TRY(get(rk->cvar_lo, d_rlo, rgl)); HIP_TRY(get(rk->counts, d_rcnt, r_inst * 4));
        }
        if (sl) {      /* behind k_rollout_risk on the same stream: the candidates' risk is this kernel's input */
            hipLaunchKernelGGL(k_plan_select, dim3(sel_grid), dim3(64 * SEL_WAVES), 0, sq, sa);
            HIP_TRY(hipGetLastError());
            if (n_pol && (si.u_choice || si.u0_choice)) {
                hipLaunchKernelGGL(k_select_inputs, dim3(sel_grid), dim3(64 * SEL_WAVES), 0, sq, si);
                HIP_TRY(hipGetLastError());
            }
            if (keep_sel) {      /* device to device from the call's temporaries, behind the kernels that wrote them */
                HIP_TRY(hipMemcpyAsync(kept.choice, d_schoice, sizeof(int) * (size_t)batch, hipMemcpyDeviceToDevice, sq));
                if (s_seq) HIP_TRY(hipMemcpyAsync(kept.u, d_such, sizeof(double) * s_seq, hipMemcpyDeviceToDevice, sq));
                hipLaunchKernelGGL(k_selection_policy, dim3(profile_grid((long long)batch)), dim3(256), 0, sq, (long long)batch, sl->P - n_pol, (const int *)d_schoice.get(), kept.policy.get());
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(get(sl->choice, d_schoice, (size_t)batch)); HIP_TRY(get(sl->score, d_sscore, (size_t)batch)); HIP_TRY(get(sl->n_admissible, d_snadm, (size_t)batch));
            HIP_TRY(get(sl->admissible, d_sadm, r_inst)); HIP_TRY(get(sl->u_choice, d_such, s_seq)); HIP_TRY(get(sl->u0_choice, d_su0, (size_t)batch * nu));
        }
        HIP_TRY(get(x_out, d_x, cx)); HIP_TRY(get(v_out, d_v, cv)); HIP_TRY(get(y_out, d_y, cy)); HIP_TRY(get(cons_vio_out, d_vio, ck)); HIP_TRY(get(cons_row_out, d_row, ck));
        HIP_TRY(get(cost_out, d_cost, T)); HIP_TRY(get(mu_total_out, d_mu, T)); HIP_TRY(get(worst_vio_out, d_wv, T));
        HIP_TRY(get(worst_step_out, d_ws, T)); HIP_TRY(get(steps_done_out, d_sd, T)); HIP_TRY(get(end_status_out, d_es, T));
        if (pc) HIP_TRY(get(pc->switches_out, d_sw, T));
        if (n_pol) HIP_TRY(get(sl->switches_out, d_sw, T));
        if (kc) {
            HIP_TRY(get(kc->sum, d_ksum, tq)); HIP_TRY(get(kc->min, d_kmin, tq)); HIP_TRY(get(kc->max, d_kmax, tq)); HIP_TRY(get(kc->min_step, d_kmins, tq));
            HIP_TRY(get(kc->max_step, d_kmaxs, tq)); HIP_TRY(get(kc->n_above, d_kabove, tq)); HIP_TRY(get(kc->n_changes, d_kchg, tq)); HIP_TRY(get(kc->n_vio, d_knvio, T));
        }
        HIP_TRY(hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, sq));
        if (sc) {
            if (keep_rows) HIP_TRY(hipMemcpyAsync(d_old, p->bat.warm, warm_len, hipMemcpyDeviceToDevice, sq));
            hipLaunchKernelGGL(k_warm_from_rollout, dim3((unsigned)((warm_len + 255) / 256)), dim3(256), 0, sq, (long long)batch, p->nb, nv, p->d_bins.get(), d_v.get(),
                               Kz * nv, d_es.get(), keep_rows ? d_old.get() : nullptr, p->bat.warm.get(), d_src.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(src_host.data(), d_src, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToHost, sq));
        }
        return MLD_OK;
    };
    /* ---- the device completion (rollout.inc: DEVICE COMPLETION): the trajectories the first kernel declined (cnt[3] of them) finished in HBM, before anything
     * reads a trajectory's result.  The list, table, marks and steps are temporaries sized by the number declined.  The resolver's resident batch supplies the
     * slots: a listed trajectory takes a slot of ITS model, a list longer than the slots of a model is solved in chunks; the inputs and results the slots
     * held are put back at the end.  A resolver whose resident batch is not the one laid out for this handle's is laid out as mld_sim_step_resolve lays it out
     * (the stepped handle's size and model_idx, by the same test): every model the list needs then has a slot. */
    auto complete = [&]() -> int {
        const size_t L = (size_t)cnt[3], nA = (size_t)aux->n, PS = (size_t)(sl ? sl->P : 1) * (size_t)S;
        const hipStream_t aq = aux->stream;
        DevBuf<long long> d_list; DevBuf<unsigned long long> d_ln; DevBuf<double> d_ans, d_ztab; DevBuf<int> d_mark, d_step, d_ent, d_slot;
        HIP_TRY(d_list.alloc(L)); HIP_TRY(d_ln.alloc(1)); HIP_TRY(d_ans.alloc(std::max<size_t>(1, L * Kz * nA))); HIP_TRY(d_mark.alloc(L * Kz));
        HIP_TRY(d_step.alloc(L)); HIP_TRY(d_ent.alloc(L)); HIP_TRY(d_slot.alloc(L));
        unsigned long long ln = 0;
        std::vector<long long> list(L);
        auto collect = [&]() -> int {
            HIP_TRY(hipMemsetAsync(d_ln, 0, sizeof(ln), sq));
            HIP_TRY(hipMemsetAsync(d_mark, 0, sizeof(int) * L * Kz, sq));
            hipLaunchKernelGGL(k_ro_collect, dim3(profile_grid((long long)T)), dim3(256), 0, sq, (long long)T, (const int *)d_es.get(), (long long)L, d_list.get(), d_ln.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&ln, d_ln, sizeof(ln), hipMemcpyDeviceToHost, sq));
            HIP_TRY(hipMemcpyAsync(list.data(), d_list, sizeof(long long) * L, hipMemcpyDeviceToHost, sq));
            return MLD_OK;
        };
        if (int rc = queue_and_wait(sq, collect)) return rc;
        if (ln != L) { mld_set_error("%s: internal: %llu trajectories ended declined, the rollout kernel counted %zu", who, ln, L); return MLD_ERR_INVALID; }
        std::sort(list.begin(), list.end());      /* (the kernel's order is the atomics': sorted, the slots are the same from call to call) */
        std::vector<int> pm, emodel(L, 0);
        if (p->has_midx) {
            pm.resize((size_t)batch);
            HIP_TRY(hipMemcpy(pm.data(), p->bat.model_idx, sizeof(int) * (size_t)batch, hipMemcpyDeviceToHost));
            for (size_t e = 0; e < L; ++e) emodel[e] = pm[(size_t)list[e] / PS];
        }
        /* the resolver's slots by model */
        std::vector<std::vector<int>> by((size_t)p->n_models);
        auto read_layout = [&]() -> int {
            std::vector<int> am((size_t)aux->batch, 0);
            if (aux->has_midx) HIP_TRY(hipMemcpy(am.data(), aux->bat.model_idx, sizeof(int) * am.size(), hipMemcpyDeviceToHost));
            for (auto &l : by) l.clear();
            for (int i = 0; i < aux->batch; ++i) by[(size_t)am[(size_t)i]].push_back(i);
            return MLD_OK;
        };
        const bool fresh = aux->batch != batch || aux->aux_src_gen != p->batch_gen || aux->aux_own_gen != aux->batch_gen;      /* mld_sim_step_resolve's test */
        if (!fresh) { if (int rc = read_layout()) return rc; }
        const size_t anx = (size_t)aux->nx, anw = (size_t)aux->nW;
        if (fresh) {
            if (int rc = lay_out_batch(aux, batch, pm.empty() ? nullptr : pm.data(), nullptr)) return rc;
            aux->aux_src_gen = p->batch_gen; aux->aux_own_gen = aux->batch_gen;
            HIP_TRY(hipMemset(aux->bat.x0, 0, sizeof(double) * (size_t)batch * anx));
            HIP_TRY(hipMemset(aux->bat.omega, 0, sizeof(double) * (size_t)batch * anw));
            if (int rc = read_layout()) return rc;
        }
        /* what the slots hold: put back when the rounds are over */
        const size_t ab = (size_t)aux->batch;
        DevBuf<double> s_x0, s_om, s_v, s_obj, s_lb; DevBuf<int> s_st, s_nd, s_pv;
        auto copy_state = [&](bool save) -> int {
            auto cp = [&](auto &keep, auto &live, size_t count) -> hipError_t {
                if (!count) return hipSuccess;
                return save ? hipMemcpyAsync(keep.get(), live.get(), sizeof(*keep.get()) * count, hipMemcpyDeviceToDevice, aq)
                            : hipMemcpyAsync(live.get(), keep.get(), sizeof(*keep.get()) * count, hipMemcpyDeviceToDevice, aq);
            };
            HIP_TRY(cp(s_x0, aux->bat.x0, ab * anx)); HIP_TRY(cp(s_om, aux->bat.omega, ab * anw)); HIP_TRY(cp(s_v, aux->bat.v, ab * nA));
            HIP_TRY(cp(s_obj, aux->bat.obj, ab)); HIP_TRY(cp(s_lb, aux->bat.lbnd, ab)); HIP_TRY(cp(s_st, aux->bat.status, ab));
            HIP_TRY(cp(s_nd, aux->bat.nodes, ab)); HIP_TRY(cp(s_pv, aux->bat.pivots, ab));
            return MLD_OK;
        };
        if (!fresh) {
            HIP_TRY(s_x0.alloc(std::max<size_t>(1, ab * anx))); HIP_TRY(s_om.alloc(std::max<size_t>(1, ab * anw))); HIP_TRY(s_v.alloc(std::max<size_t>(1, ab * nA)));
            HIP_TRY(s_obj.alloc(ab)); HIP_TRY(s_lb.alloc(ab)); HIP_TRY(s_st.alloc(ab)); HIP_TRY(s_nd.alloc(ab)); HIP_TRY(s_pv.alloc(ab));
            if (int rc = queue_and_wait(aq, [&]() -> int { return copy_state(true); })) return rc;
        }
        /* the re-run kernel's view of the call: the superset body's arguments (rollout.inc) */
        RoCandDev rcd = cd; RoCandPolDev rcq = cq;
        if (!n_pol) {
            rcq.tab_len = ptab_len; rcq.n_models = p->n_models;
            if (pc) { rcq.tab = p->pol_tab; rcq.n_seq = 0; }
            else {      /* open loop: the table whose every channel is passed through (all zero: mode 0) */
                const size_t zl = std::max<size_t>(1, (size_t)p->n_models * ptab_len);
                HIP_TRY(d_ztab.alloc(zl)); HIP_TRY(hipMemset(d_ztab, 0, sizeof(double) * zl));
                rcq.tab = d_ztab; rcq.n_seq = sl ? sl->P : 1;
            }
            if (!sl) { rcd.P = 1; rcd.plan_first = 0; rcd.u_cand = nullptr; }
        }
        RoFixDev fx{};
        fx.ent = d_ent; fx.slot = d_slot; fx.list = d_list; fx.ans = d_ans; fx.mark = d_mark; fx.ax0 = aux->bat.x0; fx.aom = aux->bat.omega; fx.step = d_step;
        fx.sel = sl ? 1 : 0;
        const void *redo_kernel = kc ? (const void *)k_rollout_redo_kpi : (const void *)k_rollout_redo;
        if (lds_bytes > 48 * 1024) HIP_TRY(hipFuncSetAttribute(redo_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        HIP_TRY(hipMemcpy(d_list, list.data(), sizeof(long long) * L, hipMemcpyHostToDevice));
        std::vector<int> hstep(L, 0), ent, slot, rest, later, todo;
        std::vector<char> open(L, 1);
        long long rounds = 0, dense = 0;
        auto run = [&]() -> int {
            for (int r = 0; r <= K; ++r) {      /* pass r leaves a trajectory declined at a step >= r: K rounds at the most, and the pass that ends them all */
                rest.clear();
                for (size_t e = 0; e < L; ++e) if (open[e]) rest.push_back((int)e);
                if (rest.empty()) break;
                SmShape Sr = SS;
                if ((p->ro_mode & MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY) && r > 0) Sr.max_pivots = aux->opts.max_pivots;      /* the cap: the first kernel's, and the pass that finds its declines again */
                bool solved = false;
                while (!rest.empty()) {      /* a chunk: as many of the rest as the resolver has slots of their models */
                    std::vector<size_t> used((size_t)p->n_models, 0);
                    ent.clear(); slot.clear(); later.clear(); todo.clear();
                    for (int e : rest) {
                        const size_t mdl = (size_t)emodel[(size_t)e];
                        if (used[mdl] < by[mdl].size()) { ent.push_back(e); slot.push_back(by[mdl][used[mdl]++]); } else later.push_back(e);
                    }
                    fx.n_items = (long long)ent.size();
                    auto redo = [&]() -> int {
                        HIP_TRY(hipMemcpyAsync(d_ent, ent.data(), sizeof(int) * ent.size(), hipMemcpyHostToDevice, sq));
                        HIP_TRY(hipMemcpyAsync(d_slot, slot.data(), sizeof(int) * slot.size(), hipMemcpyHostToDevice, sq));
                        const dim3 rg((unsigned)((ent.size() + SM_WAVES - 1) / SM_WAVES));
                        if (kc) hipLaunchKernelGGL(k_rollout_redo_kpi, rg, dim3(SM_NT), lds_bytes, sq, Sr, P, a, rcd, pd, rcq, kd, fx);
                        else hipLaunchKernelGGL(k_rollout_redo, rg, dim3(SM_NT), lds_bytes, sq, Sr, P, a, rcd, pd, rcq, fx);
                        HIP_TRY(hipGetLastError());
                        HIP_TRY(hipMemcpyAsync(hstep.data(), d_step, sizeof(int) * L, hipMemcpyDeviceToHost, sq));      /* (the number still declined, read between the rounds) */
                        return MLD_OK;
                    };
                    if (int rc = queue_and_wait(sq, redo)) return rc;
                    for (size_t i = 0; i < ent.size(); ++i) {
                        if (hstep[(size_t)ent[i]] >= 0) todo.push_back(slot[i]); else open[(size_t)ent[i]] = 0;
                    }
                    if (!todo.empty()) {
                        if (r == K) { mld_set_error("%s: internal: a trajectory is still declined after K = %d completion rounds (every round moves its declining step forward)", who, K); return MLD_ERR_INVALID; }
                        if (int rc = rollout_solve_slots(aux, todo)) return rc;
                        auto merge = [&]() -> int {
                            hipLaunchKernelGGL(k_ro_fix_merge, dim3((unsigned)std::min<size_t>(ent.size(), 65535)), dim3(64), 0, sq, (long long)ent.size(), (const int *)d_ent.get(),
                                               (const int *)d_slot.get(), (const int *)d_step.get(), K, (int)nA, (const double *)aux->bat.v.get(), nA, (const int *)aux->bat.status.get(),
                                               (const double *)aux->bat.obj.get(), d_ans.get(), d_mark.get());
                            HIP_TRY(hipGetLastError());
                            return MLD_OK;
                        };
                        if (int rc = queue_and_wait(sq, merge)) return rc;
                        dense += (long long)todo.size(); solved = true;
                    }
                    rest.swap(later);
                }
                rounds += solved ? 1 : 0;
            }
            return MLD_OK;
        };
        const int rc = run();
        int rc2 = MLD_OK;
        if (!fresh) { rc2 = queue_and_wait(aq, [&]() -> int { return copy_state(false); }); }
        long long left = 0;
        for (size_t e = 0; e < L; ++e) left += open[e] ? 1 : 0;
        p->ro_stats[0] = rounds; p->ro_stats[1] = (long long)L - left; p->ro_stats[2] = dense; p->ro_stats[3] = left;
        return rc ? rc : rc2;
    };
    auto queue = [&]() -> int { if (int rc = queue_rollout()) return rc; return queue_readers(); };
    std::fill(p->ro_stats, p->ro_stats + 4, 0LL);
    if (!dev_complete) {
        if (int rc = queue_and_wait(sq, queue)) return rc;
    } else {
        auto first = [&]() -> int {
            if (int rc = queue_rollout()) return rc;
            HIP_TRY(hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, sq));      /* (read between the rounds, as launch_small reads its counter) */
            return MLD_OK;
        };
        if (int rc = queue_and_wait(sq, first)) return rc;
        if (cnt[3]) { if (int rc = complete()) return rc; }
        if (int rc = queue_and_wait(sq, queue_readers)) return rc;
    }
    if (sc) {      /* the start is set; written / kept / none counted from the sources */
        p->has_warm = true;
        int64_t n[3] = {0, 0, 0};
        for (int32_t s : src_host) ++n[s == WS_WRITTEN ? 0 : (s == WS_KEPT ? 1 : 2)];
        if (sc->source_out) std::copy(src_host.begin(), src_host.end(), sc->source_out);
        if (sc->stats) { sc->stats[0] = (int64_t)T; sc->stats[1] = n[0]; sc->stats[2] = n[1]; sc->stats[3] = n[2]; }
    }
    if (stats) { stats[0] = (int64_t)T; stats[1] = (int64_t)cnt[1]; stats[2] = (int64_t)cnt[2]; stats[3] = (int64_t)cnt[3]; }
    if (keep_sel) {      /* the call has succeeded: its selection is the kept one, stamped with the inputs it was made for */
        kept.K = K; kept.batch = batch; kept.has = true; kept.batch_gen = p->batch_gen; kept.chain = p->chain_gen;
        p->sel = std::move(kept);
    }
    return MLD_OK;
}

extern "C" {

/* The sticky completion mode of a stepped handle: what every later call of the rollout family on it does with the trajectories its LDS solver declines
 * (rollout.inc: DEVICE COMPLETION).  0: as ever -- they end 2.  Nothing is queued; an unknown bit is refused and the mode stays. */
int mld_set_rollout_completion(mld_problem_t *p, int mode)
{
    static const char who[] = "mld_set_rollout_completion";
    if (!p) { mld_set_error("%s: p is NULL", who); return MLD_ERR_INVALID; }
    if (mode & ~RO_MODE_ALL) { mld_set_error("%s: mode = %d has unknown bits (MLD_ROLLOUT_COMPLETE_DEVICE = 1, MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY = 2)", who, mode); return MLD_ERR_INVALID; }
    p->ro_mode = mode;
    return MLD_OK;
}

/* What the last call of the rollout family on p did: out = [rounds, finished_on_device, dense_solves, left_declined]; all 0 after a call that completed nothing */
int mld_rollout_completion_stats(mld_problem_t *p, int64_t out[4])
{
    static const char who[] = "mld_rollout_completion_stats";
    if (!p) { mld_set_error("%s: p is NULL", who); return MLD_ERR_INVALID; }
    if (!out) { mld_set_error("%s: out is NULL (rounds, finished_on_device, dense_solves, left_declined)", who); return MLD_ERR_INVALID; }
    for (int k = 0; k < 4; ++k) out[k] = (int64_t)p->ro_stats[k];
    return MLD_OK;
}

/* The a-posteriori step of a scenario-based controller: what the hybrid plant does over the next K steps if the plan's (or the caller's) inputs are applied
 * and the disturbance turns out to be realisation c -- the reference's MldModel.lsim / lsim_k in a loop (models/mld_model.py:543-642, 647-699) with
 * _compute_aux (:701-766) at every step, for batch x S trajectories in ONE launch.  Everything is tested on the host before anything is queued; the call
 * reads p's current x0 and writes nothing a solve reads -- inputs, plan, MIP start, log and resident starts stay (the what-if of mld_sim_step_*) -- and
 * nothing on the resolver's handle: the kernel reads the resolver's per-model data only.  Host-synchronous. */
int mld_rollout_batch(mld_problem_t *p, mld_problem_t *aux, int K, int S, const double *u_seq, const double *omega_seq, const int64_t *start, int step,
                      const double *cost_w, int cost_rows, double *x_out, double *v_out, double *y_out, double *cons_vio_out, int32_t *cons_row_out,
                      double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out, int32_t *end_status_out,
                      int64_t stats[4])
{
    static const char who[] = "mld_rollout_batch";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const RolloutOut out{x_out, v_out, y_out, cons_vio_out, cons_row_out, cost_out, mu_total_out, worst_vio_out, worst_step_out, steps_done_out, end_status_out, stats};
    return rollout_impl(who, nullptr, p, aux, K, S, u_seq, omega_seq, start, step, cost_w, cost_rows, out);
}

/* mld_rollout_batch (policy == 0) or mld_rollout_policy (policy != 0) with the column statistics of every trajectory reduced inside the kernel
 * (k_rollout_kpi / k_rollout_policy_kpi): rollout_impl with a KpiCall, so every refusal of the two is made by the same code. */
int mld_rollout_kpi(mld_problem_t *p, mld_problem_t *aux, int policy, int K, int S, const double *u_seq, const double *u_prev, const double *omega_seq,
                    const int64_t *start, int step, const double *cost_w, int cost_rows, int n_kpi,
                    const double *w_x, const double *w_v, const double *w_y, const double *w_omega, const double *w_xk1,
                    const int32_t *price_chan, const double *thresh, double vio_tol, const int64_t *price_start,
                    double *x_out, double *v_out, double *y_out, double *cons_vio_out, int32_t *cons_row_out,
                    double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out, int32_t *end_status_out,
                    int32_t *switches_out, int64_t stats[4],
                    double *sum, double *min, double *max, int32_t *min_step, int32_t *max_step, int32_t *n_above, int32_t *n_changes, int32_t *n_vio)
{
    static const char who[] = "mld_rollout_kpi";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const PolicyCall pc{u_prev, switches_out};
    const RolloutOut out{x_out, v_out, y_out, cons_vio_out, cons_row_out, cost_out, mu_total_out, worst_vio_out, worst_step_out, steps_done_out, end_status_out, stats};
    const KpiCall kc{n_kpi, {w_x, w_v, w_y, w_omega, w_xk1}, price_chan, thresh, vio_tol, price_start, sum, min, max, min_step, max_step, n_above, n_changes, n_vio};
    return rollout_impl(who, policy ? &pc : nullptr, p, aux, K, S, u_seq, omega_seq, start, step, cost_w, cost_rows, out, nullptr, &kc);
}

/* mld_rollout_kpi (n_kpi >= 1) or the plain rollouts (n_kpi == 0: no table, the KPI arguments are ignored) with the statistics across the realisations of every
 * instance reduced on the device behind the rollout (k_rollout_risk): rollout_impl with a RiskCall, so every refusal of the others is made by the same code. */
int mld_rollout_risk(mld_problem_t *p, mld_problem_t *aux, int policy, int K, int S, const double *u_seq, const double *u_prev, const double *omega_seq,
                     const int64_t *start, int step, const double *cost_w, int cost_rows, int n_kpi,
                     const double *w_x, const double *w_v, const double *w_y, const double *w_omega, const double *w_xk1,
                     const int32_t *price_chan, const double *thresh, double vio_tol, const int64_t *price_start,
                     double *x_out, double *v_out, double *y_out, double *cons_vio_out, int32_t *cons_row_out,
                     double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out, int32_t *end_status_out,
                     int32_t *switches_out, int64_t stats[4],
                     double *sum, double *min, double *max, int32_t *min_step, int32_t *max_step, int32_t *n_above, int32_t *n_changes, int32_t *n_vio,
                     int G, const int32_t *col_src, const int32_t *col_q, const double *level, int L, const double *alpha,
                     double *r_mean, double *r_min, double *r_max, int32_t *r_min_c, int32_t *r_max_c, int32_t *r_n_exceed,
                     double *r_quantile, int32_t *r_quantile_c, double *r_cvar_hi, double *r_cvar_lo, int32_t *counts)
{
    static const char who[] = "mld_rollout_risk";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const PolicyCall pc{u_prev, switches_out};
    const RolloutOut out{x_out, v_out, y_out, cons_vio_out, cons_row_out, cost_out, mu_total_out, worst_vio_out, worst_step_out, steps_done_out, end_status_out, stats};
    const KpiCall kc{n_kpi, {w_x, w_v, w_y, w_omega, w_xk1}, price_chan, thresh, vio_tol, price_start, sum, min, max, min_step, max_step, n_above, n_changes, n_vio};
    const RiskCall rk{G, col_src, col_q, level, L, alpha, r_mean, r_min, r_max, r_min_c, r_max_c, r_n_exceed, r_quantile, r_quantile_c, r_cvar_hi, r_cvar_lo, counts};
    return rollout_impl(who, policy ? &pc : nullptr, p, aux, K, S, u_seq, omega_seq, start, step, cost_w, cost_rows, out, nullptr, n_kpi ? &kc : nullptr, &rk);
}

/* mld_rollout_risk's open loop over P candidate input sequences per instance under the same S realisations (k_rollout_cand / k_rollout_cand_kpi), each
 * candidate's risk reduced by k_rollout_risk, and per instance the admissible candidate of least objective statistic chosen by k_plan_select behind it
 * (plan_select.inc: THE RULE): rollout_impl with a SelectCall, so every refusal of the others is made by the same code. */
int mld_rollout_select(mld_problem_t *p, mld_problem_t *aux, int K, int S, int P, int plan_first, const double *u_cand, const double *omega_seq,
                       const int64_t *start, int step, const double *cost_w, int cost_rows, int n_kpi,
                       const double *w_x, const double *w_v, const double *w_y, const double *w_omega, const double *w_xk1,
                       const int32_t *price_chan, const double *thresh, double vio_tol, const int64_t *price_start,
                       int G, const int32_t *col_src, const int32_t *col_q, const double *level, int L, const double *alpha,
                       int obj_col, int obj_kind, int obj_level, int n_cons, const int32_t *cons_col, const int32_t *cons_kind, const int32_t *cons_level,
                       const double *cons_bound, int min_complete,
                       int32_t *choice, double *score, int32_t *n_admissible, uint8_t *admissible, double *u_choice, double *u0_choice,
                       double *r_mean, double *r_min, double *r_max, int32_t *r_min_c, int32_t *r_max_c, int32_t *r_n_exceed,
                       double *r_quantile, int32_t *r_quantile_c, double *r_cvar_hi, double *r_cvar_lo, int32_t *counts,
                       double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out, int32_t *end_status_out,
                       int64_t stats[4],
                       double *sum, double *min, double *max, int32_t *min_step, int32_t *max_step, int32_t *n_above, int32_t *n_changes, int32_t *n_vio)
{
    static const char who[] = "mld_rollout_select";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const RolloutOut out{nullptr, nullptr, nullptr, nullptr, nullptr, cost_out, mu_total_out, worst_vio_out, worst_step_out, steps_done_out, end_status_out, stats};
    const KpiCall kc{n_kpi, {w_x, w_v, w_y, w_omega, w_xk1}, price_chan, thresh, vio_tol, price_start, sum, min, max, min_step, max_step, n_above, n_changes, n_vio};
    const RiskCall rk{G, col_src, col_q, level, L, alpha, r_mean, r_min, r_max, r_min_c, r_max_c, r_n_exceed, r_quantile, r_quantile_c, r_cvar_hi, r_cvar_lo, counts};
    const SelectCall sl{P, plan_first, u_cand, obj_col, obj_kind, obj_level, n_cons, cons_col, cons_kind, cons_level, cons_bound, min_complete,
                        choice, score, n_admissible, admissible, u_choice, u0_choice};
    return rollout_impl(who, nullptr, p, aux, K, S, nullptr, omega_seq, start, step, cost_w, cost_rows, out, nullptr, n_kpi ? &kc : nullptr, &rk, &sl);
}

/* mld_rollout_select with closed-loop rule policies among the candidates: the last T of the P candidates are ThresholdPolicy tables stepped in closed loop
 * (k_rollout_cand_policy / k_rollout_cand_policy_kpi: ro_run<true> with a table per candidate), the chosen inputs by k_select_inputs behind k_plan_select.
 * rollout_impl with the SelectCall extended, so every refusal of the others is made by the same code; T == 0 is mld_rollout_select's call.  The handle is
 * read and never changed, and nothing is finished on the host: a trajectory the LDS solver declines ends 2 and is counted. */
int mld_rollout_select_policy(mld_problem_t *p, mld_problem_t *aux, int K, int S, int P, int plan_first, const double *u_cand, const double *omega_seq,
                              const int64_t *start, int step, const double *cost_w, int cost_rows, int n_kpi,
                              const double *w_x, const double *w_v, const double *w_y, const double *w_omega, const double *w_xk1,
                              const int32_t *price_chan, const double *thresh, double vio_tol, const int64_t *price_start,
                              int G, const int32_t *col_src, const int32_t *col_q, const double *level, int L, const double *alpha,
                              int obj_col, int obj_kind, int obj_level, int n_cons, const int32_t *cons_col, const int32_t *cons_kind, const int32_t *cons_level,
                              const double *cons_bound, int min_complete,
                              int32_t *choice, double *score, int32_t *n_admissible, uint8_t *admissible, double *u_choice, double *u0_choice,
                              double *r_mean, double *r_min, double *r_max, int32_t *r_min_c, int32_t *r_max_c, int32_t *r_n_exceed,
                              double *r_quantile, int32_t *r_quantile_c, double *r_cvar_hi, double *r_cvar_lo, int32_t *counts,
                              double *cost_out, double *mu_total_out, double *worst_vio_out, int32_t *worst_step_out, int32_t *steps_done_out, int32_t *end_status_out,
                              int64_t stats[4],
                              double *sum, double *min, double *max, int32_t *min_step, int32_t *max_step, int32_t *n_above, int32_t *n_changes, int32_t *n_vio,
                              int T, const double *pol_sel, const double *pol_on_at, const double *pol_off_at, const double *pol_u_on, const double *pol_u_off,
                              const int32_t *pol_mode, const double *u_prev, int32_t *switches_out)
{
    static const char who[] = "mld_rollout_select_policy";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    const RolloutOut out{nullptr, nullptr, nullptr, nullptr, nullptr, cost_out, mu_total_out, worst_vio_out, worst_step_out, steps_done_out, end_status_out, stats};
    const KpiCall kc{n_kpi, {w_x, w_v, w_y, w_omega, w_xk1}, price_chan, thresh, vio_tol, price_start, sum, min, max, min_step, max_step, n_above, n_changes, n_vio};
    const RiskCall rk{G, col_src, col_q, level, L, alpha, r_mean, r_min, r_max, r_min_c, r_max_c, r_n_exceed, r_quantile, r_quantile_c, r_cvar_hi, r_cvar_lo, counts};
    const SelectCall sl{P, plan_first, u_cand, obj_col, obj_kind, obj_level, n_cons, cons_col, cons_kind, cons_level, cons_bound, min_complete,
                        choice, score, n_admissible, admissible, u_choice, u0_choice, T, pol_sel, pol_on_at, pol_off_at, pol_u_on, pol_u_off, pol_mode, u_prev, switches_out};
    return rollout_impl(who, nullptr, p, aux, K, S, nullptr, omega_seq, start, step, cost_w, cost_rows, out, nullptr, n_kpi ? &kc : nullptr, &rk, &sl);
}

} // extern "C"
