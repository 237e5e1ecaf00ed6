// Solve path of the resident batch: upload, constraint blocks, right-hand sides, launch / finish, downloads, MIP start, cutoffs, hand-off settings,
// open nodes, staged inputs, mld_rhs_batch and the debug hooks.
extern "C" {

/* instances grouped by model (stable counting sort) and cut into workgroup-sized chunks: the batch as the N dimension of one GEMM
 * per model.  perm is empty when the instances of every model are already contiguous in order (model_idx == NULL). */
static void build_rhs_groups(const int32_t *model_idx, int batch, int n_models, std::vector<int> &perm, std::vector<RhsGroup> &groups)
{
    perm.clear(); groups.clear();
    if (!model_idx) {
        for (int s = 0; s < batch; s += RM_NI) groups.push_back(RhsGroup{0, s, std::min(RM_NI, batch - s)});
        return;
    }
    std::vector<int> cnt(n_models + 1, 0);
    for (int b = 0; b < batch; ++b) cnt[model_idx[b] + 1]++;
    for (int k = 0; k < n_models; ++k) cnt[k + 1] += cnt[k];
    perm.resize(batch);
    std::vector<int> pos(cnt.begin(), cnt.end() - 1);
    for (int b = 0; b < batch; ++b) perm[pos[model_idx[b]]++] = b;
    for (int k = 0; k < n_models; ++k)
        for (int s = cnt[k]; s < cnt[k + 1]; s += RM_NI) groups.push_back(RhsGroup{k, s, std::min(RM_NI, cnt[k + 1] - s)});
}

static bool rhs_mfma_fits(int nx, int nW) { return ((nx + nW + 3) & ~3) <= RM_KMAX; }

/* launch of a member of the instance-GEMM family (mfma.inc): kern<F32>, a workgroup per RhsGroup */
#define LAUNCH_INST_GEMM(kern, f32, n_groups, lds, stream, ...) do {                                                             \
    if (f32) hipLaunchKernelGGL(kern<true>, dim3(n_groups), dim3(64 * RM_WAVES), lds, stream, __VA_ARGS__);                      \
    else hipLaunchKernelGGL(kern<false>, dim3(n_groups), dim3(64 * RM_WAVES), lds, stream, __VA_ARGS__); } while (0)
static void launch_rhs_mfma(bool f32, int n_groups, int m0, int nx, int nW, const double *Hx, const double *Hw, const double *H5, const double *rs,
                            const RhsGroup *groups, const int *perm, const double *x0, const double *omega, double *hs, hipStream_t stream = 0)
{
    const int Kp = (nx + nW + 3) & ~3;
    const size_t lds = sizeof(double) * 16 * (size_t)(Kp + 1);
    LAUNCH_INST_GEMM(k_rhs_mfma, f32, n_groups, lds, stream, m0, nx, nW, Kp, Hx, Hw, H5, rs, groups, perm, x0, omega, hs);
}

/* a batch laid out on the handle: buffers, model_idx, RHS groups, fixings -- everything of mld_upload_batch but the inputs themselves, which the caller of
 * this function fills (mld_upload_batch from the host, mld_sim_step_resolve on the device) */
static int lay_out_batch(mld_problem_t *p, int batch, const int32_t *model_idx, const uint8_t *fixed_bin)
{
    if (model_idx) for (int b = 0; b < batch; ++b) if (model_idx[b] < 0 || model_idx[b] >= p->n_models) { mld_set_error("model_idx[%d]=%d out of range", b, model_idx[b]); return MLD_ERR_INVALID; }
    int rc = ensure_batch(p, batch);
    if (rc) { p->batch = 0; return rc; }
    p->batch = batch; p->has_midx = model_idx != nullptr; p->has_fixed = fixed_bin != nullptr;
    inputs_new_batch(p);
    p->all_fixed = false;
    if (fixed_bin && p->nb) { bool all = true; const size_t tot = (size_t)batch * p->nb; for (size_t k = 0; k < tot && all; ++k) all = fixed_bin[k] != 255; p->all_fixed = all; }
    if (p->order_batch != batch) p->order_batch = 0;
    {
        std::vector<int> perm; std::vector<RhsGroup> groups;
        build_rhs_groups(model_idx, batch, p->n_models, perm, groups);
        p->bat.perm.reset(); p->bat.groups.reset();
        p->n_groups = (int)groups.size();
        if ((rc = upload(p->bat.perm, perm)) || (rc = upload(p->bat.groups, groups))) return rc;
    }
    if (model_idx) HIP_TRY(hipMemcpy(p->bat.model_idx, model_idx, sizeof(int) * batch, hipMemcpyHostToDevice));
    if (fixed_bin && p->nb) HIP_TRY(hipMemcpy(p->bat.fixed, fixed_bin, (size_t)batch * p->nb, hipMemcpyHostToDevice));
    return MLD_OK;
}

int mld_upload_batch(mld_problem_t *p, int batch, const int32_t *model_idx, const double *x0, const double *omega,
                     const uint8_t *fixed_bin)
{
    if (int rc = entry_guard(p, "mld_upload_batch", false, nullptr)) return rc;
    if (!p || batch < 1) { mld_set_error("mld_upload_batch: bad arguments"); return MLD_ERR_INVALID; }
    if ((p->nx && !x0) || (p->nW && !omega)) { mld_set_error("mld_upload_batch: x0/omega required"); return MLD_ERR_INVALID; }
    if (int rc = lay_out_batch(p, batch, model_idx, fixed_bin)) return rc;
    if (p->nx) HIP_TRY(hipMemcpy(p->bat.x0, x0, sizeof(double) * (size_t)batch * p->nx, hipMemcpyHostToDevice));
    if (p->nW) HIP_TRY(hipMemcpy(p->bat.omega, omega, sizeof(double) * (size_t)batch * p->nW, hipMemcpyHostToDevice));
    return MLD_OK;
}

int mld_upload_constraint_blocks_x(mld_problem_t *p, int n_cols, const double *omega_cols, const int32_t *col_rows, const double *x_cols)
{
    if (int rc = entry_guard(p, "mld_upload_constraint_blocks", false, "upload the batch first")) return rc;
    if (n_cols < 0 || (n_cols > 0 && p->nW && !omega_cols)) { mld_set_error("mld_upload_constraint_blocks: bad arguments"); return MLD_ERR_INVALID; }
    if (int rc = check_col_rows(p, nullptr, n_cols, col_rows)) return rc;
    p->n_xcols = 0;
    if (n_cols == 0 || !p->nW) return MLD_OK;
    const bool with_x = x_cols && p->nx;
    if (int rc = stage_xcols(p, n_cols, col_rows != nullptr, with_x)) return rc;
    HIP_TRY(hipMemcpy(p->bat.xcols, omega_cols, sizeof(double) * (size_t)p->batch * n_cols * p->nW, hipMemcpyHostToDevice));
    if (col_rows) HIP_TRY(hipMemcpy(p->bat.xrows, col_rows, sizeof(int) * n_cols, hipMemcpyHostToDevice));
    if (with_x) HIP_TRY(hipMemcpy(p->bat.xcols_x, x_cols, sizeof(double) * (size_t)p->batch * n_cols * p->nx, hipMemcpyHostToDevice));
    p->n_xcols = n_cols;
    return MLD_OK;
}

int mld_upload_constraint_blocks(mld_problem_t *p, int n_cols, const double *omega_cols, const int32_t *col_rows)
{
    return mld_upload_constraint_blocks_x(p, n_cols, omega_cols, col_rows, nullptr);
}

/* LDS-resident LP path -- relaxation-only mode: every binary fixed -> one LP per instance, solved in LDS (k_lp_lds); right-hand sides with the
 * Toeplitz row scales.  Runs to completion: redo lists the instances whose working basis outgrew LDS (status -1), for the dense kernel. */
static int launch_lds_lp(mld_problem *p, std::vector<int> &redo)
{
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    const mld_model *t = p->tight.get();
    launch_rhs_mfma((p->opts.flags & MLD_F32) != 0, p->n_groups, p->m0, p->nx, p->nW, t->d_out[O_HX], t->d_out[O_HW], t->d_out[O_H5], p->d_rs_t,
                    p->bat.groups, p->bat.perm, p->bat.x0, p->bat.omega, p->bat.hs, sq);
    if (p->n_xcols > 0)
        hipLaunchKernelGGL(k_rhs_extra, dim3(batch), dim3(256), 0, sq, p->m0, p->nx, p->nW, t->d_out[O_HX], t->d_out[O_HW], t->d_out[O_H5],
                           p->d_rs_t, p->has_midx ? p->bat.model_idx.get() : nullptr, p->bat.x0, p->bat.xcols, p->n_xcols, p->bat.xrows, p->bat.hs, p->has_xcols_x ? p->bat.xcols_x.get() : nullptr);
    if (p->ic_ld) {      /* per-instance cost under the Toeplitz-compatible column scales, and its constant at the current inputs */
        if (!p->bat.qs_inst_t) HIP_TRY(p->bat.qs_inst_t.alloc((size_t)batch * std::max(1, p->n)));
        if (int rc = launch_instance_cost(p, p->d_cs, p->bat.qs_inst, p->bat.rconst, p->d_cs_t, p->bat.qs_inst_t)) return rc;
    }
    HIP_TRY(hipEventRecord(p->ev[1], sq));
    LpModelDev LM; LM.blk = p->d_blk_t; LM.qs = p->d_qs_t; LM.lb = p->d_lb_t; LM.ub = p->d_ub_t; LM.cs = p->d_cs_t;
    LM.cx = p->nx ? p->d_cx.get() : nullptr; LM.cw = p->nW ? p->d_cw.get() : nullptr; LM.c0 = p->d_c0; LM.bins = p->d_bins; LM.nb = p->nb; LM.is_int = p->d_is_int;
    LpBatchDev LB; LB.batch = batch; LB.model_idx = p->has_midx ? p->bat.model_idx.get() : nullptr; LB.x0 = p->bat.x0; LB.omega = p->bat.omega; LB.hs = p->bat.hs;
    LB.fixed = p->bat.fixed; LB.v_out = p->bat.v; LB.obj_out = p->bat.obj; LB.lb_out = p->bat.lbnd; LB.status_out = p->bat.status; LB.nodes_out = p->bat.nodes;
    LB.pivots_out = p->bat.pivots; LB.ticks_out = p->bat.ticks; LB.prof_out = p->bat.prof; LB.counter = p->d_counter; LB.cuts_out = p->bat.cuts;
    LB.qs_inst = p->ic_ld ? p->bat.qs_inst_t.get() : nullptr; LB.rconst = p->ic_ld ? p->bat.rconst.get() : nullptr;
    p->LS.max_pivots = p->opts.max_pivots;
    HIP_TRY(hipMemsetAsync(p->bat.cuts, 0, sizeof(int) * batch, sq));
    HIP_TRY(hipFuncSetAttribute((const void *)k_lp_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lp_lds_bytes));
    hipLaunchKernelGGL(k_lp_lds, dim3(std::min(batch, p->lp_slots)), dim3(LP_NT), p->lp_lds_bytes, sq, p->LS, LM, LB, (unsigned char *)nullptr);
    HIP_TRY(hipMemsetAsync(p->bat.refac, 0, sizeof(int) * batch, sq));
    HIP_TRY(hipMemsetAsync(p->bat.rows, 0, sizeof(long long) * batch, sq));
    HIP_TRY(hipStreamSynchronize(sq));
    HIP_TRY(hipGetLastError());
    std::vector<int> stat(batch);
    HIP_TRY(hipMemcpy(stat.data(), p->bat.status, sizeof(int) * batch, hipMemcpyDeviceToHost));
    redo.clear();
    if (!(p->opts.reserved & MLD_DBG_LP_LDS_NO_REDO))      /* diagnostics: leave status -1 visible instead of re-solving */
        for (int i = 0; i < batch; ++i) if (stat[i] == -1) redo.push_back(i);
    return MLD_OK;
}

static ProblemDev problem_dev(const mld_problem *p);
static BatchDev batch_dev(const mld_problem *p, bool ho);
static int launch_rhs_cost(mld_problem *p);

/* Small-problem path (MLD_SMALL_LDS): the dense path's right-hand sides and cost, then k_small_milp, a wave per instance.  Runs to completion: the 4-byte
 * counter of declined instances is read, and only when it is not zero the statuses -- redo lists the declined instances (status -1), for the dense kernel. */
static int launch_small(mld_problem *p, std::vector<int> &redo)
{
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    if (int rc = launch_rhs_cost(p)) return rc;
    HIP_TRY(hipEventRecord(p->ev[1], sq));
    const ProblemDev P = problem_dev(p);
    const BatchDev B = batch_dev(p, false);
    SmShape SS = p->SS;
    SS.max_nodes = p->opts.max_nodes; SS.gap_abs = p->opts.gap_abs; SS.gap_rel = p->opts.gap_rel;
    SS.max_pivots = (p->opts.reserved & MLD_DBG_SMALL_PIVOT_CAP) ? 2 : p->opts.max_pivots;
    HIP_TRY(hipMemsetAsync(p->d_declined, 0, sizeof(int), sq));
    HIP_TRY(hipMemsetAsync(p->bat.cuts, 0, sizeof(int) * batch, sq));
    HIP_TRY(hipMemsetAsync(p->bat.refac, 0, sizeof(int) * batch, sq));
    HIP_TRY(hipMemsetAsync(p->bat.rows, 0, sizeof(long long) * batch, sq));
    if (p->small_lds_bytes > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)k_small_milp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->small_lds_bytes));
    const int grid = std::min((batch + SM_WAVES - 1) / SM_WAVES, p->small_slots);
    hipLaunchKernelGGL(k_small_milp, dim3(grid), dim3(SM_NT), p->small_lds_bytes, sq, SS, P, B, p->d_declined.get());
    int declined = 0;
    HIP_TRY(hipMemcpyAsync(&declined, p->d_declined, sizeof(int), hipMemcpyDeviceToHost, sq));
    HIP_TRY(hipStreamSynchronize(sq));
    HIP_TRY(hipGetLastError());
    redo.clear();
    if (declined) {
        std::vector<int> stat(batch);
        HIP_TRY(hipMemcpy(stat.data(), p->bat.status, sizeof(int) * batch, hipMemcpyDeviceToHost));
        for (int i = 0; i < batch; ++i) if (stat[i] == -1) redo.push_back(i);
    }
    p->small_stats[0] = batch - (long long)redo.size(); p->small_stats[1] = (long long)redo.size();
    return MLD_OK;
}

/* right-hand sides of the dense path (K3) with the extra constraint blocks, and the per-instance part of the cost (quadratic atoms, mld_upload_instance_cost) */
static int launch_rhs_cost(mld_problem *p)
{
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    const mld_model *t = p->tight.get();
    const int *midx = p->has_midx ? p->bat.model_idx.get() : nullptr;
    if (p->m0 && !p->std_block)        /* no standard block: every row starts without a right-hand side; the extra blocks' row-wise minimum follows */
        hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)(((size_t)batch * p->m0 + 255) / 256)), dim3(256), 0, sq, (size_t)batch * p->m0, 1.0e30, p->bat.hs);
    else if (p->m0 && rhs_mfma_fits(p->nx, p->nW) && !(p->opts.reserved & MLD_DBG_GEMM_VALU))     /* K3 as one GEMM per model on the matrix cores */
        launch_rhs_mfma((p->opts.flags & MLD_F32) != 0, p->n_groups, p->m0, p->nx, p->nW, t->d_out[O_HX], t->d_out[O_HW], t->d_out[O_H5], p->d_rs,
                        p->bat.groups, p->bat.perm, p->bat.x0, p->bat.omega, p->bat.hs, sq);
    else if (p->m0)
        hipLaunchKernelGGL(k_rhs, dim3(batch), dim3(256), 0, sq, p->m0, p->nx, p->nW, t->d_out[O_HX], t->d_out[O_HW], t->d_out[O_H5],
                           p->d_rs, midx, p->bat.x0, p->bat.omega, p->bat.hs, 1);
    if (p->m0 && p->n_xcols > 0)
        hipLaunchKernelGGL(k_rhs_extra, dim3(batch), dim3(256), 0, sq, p->m0, p->nx, p->nW, t->d_out[O_HX], t->d_out[O_HW], t->d_out[O_H5],
                           p->d_rs, midx, p->bat.x0, p->bat.xcols, p->n_xcols, p->bat.xrows, p->bat.hs, p->has_xcols_x ? p->bat.xcols_x.get() : nullptr);
    if (p->has_quad || p->ic_ld) return launch_instance_cost(p, p->d_cs, p->bat.qs_inst, p->bat.rconst, nullptr, nullptr);
    return MLD_OK;
}

static ProblemDev problem_dev(const mld_problem *p)
{
    const mld_model *t = p->tight.get();
    ProblemDev P;
    P.Gp = p->d_Gp; P.Gs = p->d_Gs; P.rs = p->d_rs; P.cs = p->d_cs; P.qs = p->d_qs; P.lb = p->d_lb; P.ub = p->d_ub; P.is_int = p->d_is_int;
    P.bins = p->d_bins; P.colperm = p->d_colperm; P.Hx = t->d_out[O_HX]; P.Hw = t->d_out[O_HW]; P.H5 = t->d_out[O_H5];
    P.cx = p->nx ? p->d_cx.get() : nullptr; P.cw = p->nW ? p->d_cw.get() : nullptr; P.c0 = p->d_c0;
    P.Ps = p->has_quad ? p->d_Ps.get() : nullptr;
    P.act_max = p->d_actmax;
    P.csr_ptr = p->d_csr_ptr; P.csr_col = p->d_csr_col; P.csr_val = p->d_csr_val; P.csc_ptr = p->d_csc_ptr; P.csc_row = p->d_csc_row; P.csc_val = p->d_csc_val; P.nnz_cap = p->nnz_cap;
    P.binpos = p->d_binpos;
    return P;
}

/* the resident batch as k_solve sees it; with the in-kernel hand-off (ho) the fixings and cutoffs become per-entry arrays the items write */
static BatchDev batch_dev(const mld_problem *p, bool ho)
{
    const BatchBufs &b = p->bat;
    BatchDev B;
    B.batch = p->batch; B.model_idx = p->has_midx ? b.model_idx.get() : nullptr; B.x0 = b.x0; B.omega = b.omega;
    B.fixed = p->has_fixed || ho ? b.fixed.get() : nullptr; B.hs = b.hs;
    B.warm = p->has_warm ? b.warm.get() : nullptr;
    B.cutoff = p->has_cutoff || ho ? b.cutoff.get() : nullptr;
    B.open_depth = p->want_open ? b.open_depth.get() : nullptr; B.open_var = b.open_var; B.open_val = b.open_val; B.open_flag = b.open_flag;
    const bool inst_q = p->has_quad || p->ic_ld;      /* k_solve takes the QP relaxation on S.qp && P.Ps, never on qs_inst being there */
    B.qs_inst = inst_q ? b.qs_inst.get() : nullptr; B.rconst = inst_q ? b.rconst.get() : nullptr; B.v_out = b.v; B.obj_out = b.obj; B.lb_out = b.lbnd;
    B.status_out = b.status; B.nodes_out = b.nodes; B.pivots_out = b.pivots; B.cuts_out = b.cuts; B.refac_out = b.refac;
    B.ticks_out = b.ticks; B.rows_out = b.rows; B.prof_out = b.prof; B.trace = p->d_trace;
    B.counter = p->d_counter;
    B.order = (p->order_batch == p->batch && !(p->opts.reserved & MLD_DBG_NO_ORDER)) ? b.order.get() : nullptr;
    B.ho = ho ? 1 | (p->has_fixed ? 0 : 2) : 0; B.cap = p->batch_cap; B.tail = b.ho.tail; B.finished = b.ho.finished;
    B.ho_sub_nodes = p->ho_sub_nodes > 0 ? p->ho_sub_nodes : p->opts.max_nodes; B.ho_max_gen = p->ho_max_gen; B.ho_max_children = p->ho_max_children;
    B.item_src = b.ho.item_src; B.item_root = b.ho.item_root; B.item_gen = b.ho.item_gen; B.item_label = b.ho.item_label; B.item_ready = b.ho.item_ready;
    B.item_children = b.ho.item_children;
    B.tree_count = b.ho.tree_count; B.tree_dead = b.ho.tree_dead; B.ho_max_tree = p->ho_max_tree; B.ho_donate = p->ho_donate; B.ho_rounds = p->ho_rounds;
    return B;
}

/* wait for the launched solve; the handle is unlocked whatever the outcome (every entry point refuses a problem that is in flight) */
static int wait_solve(mld_problem *p)
{
    const hipError_t ew = hipEventSynchronize(p->ev[2]);
    p->flight = Flight::idle;
    if (ew != hipSuccess) { mld_set_error("mld_solve: %s", hipGetErrorString(ew)); return MLD_ERR_HIP; }
    HIP_TRY(hipGetLastError());
    p->solved = true; p->advanced = false;
    return MLD_OK;
}

/* queue a solve of the resident batch on the problem's stream.  The dense path returns with k_solve queued (Flight::queued); the LDS path,
 * whose fall-back needs the statuses on the host, returns complete (Flight::lds_done) */
static int launch(mld_problem *p)
{
    if (!p || p->batch < 1) { mld_set_error("mld_solve_resident: nothing uploaded"); return MLD_ERR_INVALID; }
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    if (!p->ev_ok) {      /* the three timing events and the statistics buffer live as long as the problem */
        HIP_TRY(hipEventCreate(&p->ev[0])); HIP_TRY(hipEventCreate(&p->ev[1])); HIP_TRY(hipEventCreate(&p->ev[2]));
        HIP_TRY(p->d_statbuf.alloc(8));
        p->ev_ok = true;
    }
    if (p->flight != Flight::idle) { mld_set_error("mld_solve_launch: the previous launch has not been finished"); return MLD_ERR_INVALID; }
    HIP_TRY(hipMemsetAsync(p->d_counter, 0, sizeof(int), sq));
    HIP_TRY(hipEventRecord(p->ev[0], sq));
    const bool lp_path = p->lp_ok && p->all_fixed && !(p->opts.reserved & MLD_DBG_NO_LP_LDS) && p->std_block && !p->has_quad && rhs_mfma_fits(p->nx, p->nW);
    /* small-problem path (MLD_SMALL_LDS): everything k_small_milp does not do stays with the dense kernel */
    const bool small_path = p->small_ok && !lp_path && !p->has_quad && !p->ho_enable && !p->has_cutoff && !p->want_open && !(p->opts.time_limit > 0.0);
    const bool lds_path = lp_path || small_path;      /* either way: runs to completion here, the dense kernel takes what it left (redo) */
    p->small_stats[0] = p->small_stats[1] = 0;
    std::vector<int> redo;      /* LDS paths: the overflow / declined instances, re-solved by k_solve */
    int rc;
    if (lp_path && (rc = launch_lds_lp(p, redo))) return rc;
    if (small_path && (rc = launch_small(p, redo))) return rc;
    if (lds_path && redo.empty()) {
        HIP_TRY(hipEventRecord(p->ev[2], sq));
    } else {
        if (lds_path) HIP_TRY(hipMemsetAsync(p->d_counter, 0, sizeof(int), sq));
        if (!small_path && (rc = launch_rhs_cost(p))) return rc;      /* (the small path has run it: the same right-hand sides and cost) */
        if (!lds_path) HIP_TRY(hipEventRecord(p->ev[1], sq));
        p->S.qp = p->has_quad ? 1 : 0;
        const bool ho = p->ho_enable && p->bat.ho.tail && !lds_path && p->nb > 0;      /* (a quadratic cost included: items index qs_inst / rconst by their source instance, < batch) */
        const ProblemDev P = problem_dev(p);
        BatchDev B = batch_dev(p, ho);
        if (ho && (rc = handoff_reset(p))) return rc;
        if (lds_path) {      /* only the overflow instances of the LP path / the instances the small path declined */
            HIP_TRY(hipMemcpy(p->bat.order, redo.data(), sizeof(int) * redo.size(), hipMemcpyHostToDevice));
            p->order_batch = 0;
            B.order = p->bat.order; B.batch = (int)redo.size();
        }
        const int grid = ho ? p->n_slots : std::min(B.batch, p->n_slots);      /* (hand-off: the workgroups without an instance wait for items) */
        if (p->lds_bytes > 48 * 1024)   /* per-function limit: set for THIS problem (several problems of different size may be alive) */
            HIP_TRY(hipFuncSetAttribute((const void *)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds_bytes));
        hipLaunchKernelGGL(k_solve, dim3(grid), dim3(SOL_NT), p->lds_bytes, sq, p->S, P, B, p->d_ws.get());
        if (ho && (rc = handoff_merge(merge_args(p), sq))) return rc;
        p->ho_ran = ho;
        HIP_TRY(hipEventRecord(p->ev[2], sq));
    }
    if (!lds_path) { p->flight = Flight::queued; return MLD_OK; }
    if ((rc = wait_solve(p))) return rc;
    p->flight = Flight::lds_done;      /* (mld_solve_finish only reports -- the handle stays in flight until then, like a queued dense solve) */
    return MLD_OK;
}

/* wait for the launched solve and report: queue statistics, mld_stats, and the longest-first order for the next solve of this batch size */
static int finish(mld_problem *p, mld_stats *st)
{
    if (!p || p->batch < 1) { mld_set_error("mld_solve_resident: nothing uploaded"); return MLD_ERR_INVALID; }
    if (p->flight == Flight::idle) { mld_set_error("mld_solve_finish: no launched solve"); return MLD_ERR_INVALID; }
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    const bool dense = p->flight == Flight::queued;
    int rc;
    if ((rc = wait_solve(p))) return rc;
    if (dense && p->ho_ran) {      /* queue statistics of the launch that just ended */
        int tl = 0, unf = 0, fin = 0;
        HIP_TRY(hipMemcpyAsync(&tl, p->bat.ho.tail, sizeof(int), hipMemcpyDeviceToHost, sq));
        HIP_TRY(hipMemcpyAsync(&unf, p->bat.skipped, sizeof(int), hipMemcpyDeviceToHost, sq));
        HIP_TRY(hipMemcpyAsync(&fin, p->bat.ho.finished, sizeof(int), hipMemcpyDeviceToHost, sq));
        HIP_TRY(hipStreamSynchronize(sq));
        /* finished ended at tail and then took: + 1 per tree given up for its size, + 65536 per tree given up because the queue was full */
        const int extra = fin - tl;
        p->ho_stats[0] = tl - batch; p->ho_stats[1] = extra % 65536; p->ho_stats[2] = unf; p->ho_stats[3] = extra / 65536;
    }
    if (st) {
        memset(st, 0, sizeof(*st));
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, p->ev[0], p->ev[1])); HIP_TRY(hipEventElapsedTime(&b, p->ev[1], p->ev[2]));
        st->rhs_ms = a; st->solve_ms = b;
        long long h[8];
        hipLaunchKernelGGL(k_batch_stats, dim3(1), dim3(256), 0, sq, batch, p->bat.status, p->bat.nodes, p->bat.pivots, p->bat.cuts, p->bat.refac, p->d_statbuf);
        HIP_TRY(hipMemcpyAsync(h, p->d_statbuf, sizeof(h), hipMemcpyDeviceToHost, sq));
        HIP_TRY(hipStreamSynchronize(sq));
        st->nodes = h[0]; st->pivots = h[1]; st->cuts = h[2]; st->refactors = h[3];
        st->n_optimal = (int)h[4]; st->n_infeasible = (int)h[5]; st->n_node_limit = (int)h[6]; st->n_numerical = (int)h[7];
    }
    if (dense && batch > p->n_slots && !(p->opts.reserved & MLD_DBG_NO_ORDER)) {
        /* Work-queue order for the next solve of this batch size: longest first (LPT).  Consecutive MPC steps solve
         * nearly the same instances, so the previous in-kernel time predicts the next one; starting the long
         * branch-and-bound runs first removes the partially idle tail of the persistent grid.  Results do not depend
         * on the order (every instance is solved by one workgroup, bit-reproducibly). */
        std::vector<long long> ticks(batch);
        HIP_TRY(hipMemcpy(ticks.data(), p->bat.ticks, sizeof(long long) * batch, hipMemcpyDeviceToHost));
        std::vector<int> ord(batch);
        for (int i = 0; i < batch; ++i) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return ticks[a] > ticks[b]; });
        HIP_TRY(hipMemcpy(p->bat.order, ord.data(), sizeof(int) * batch, hipMemcpyHostToDevice));
        p->order_batch = batch;
    }
    return MLD_OK;
}

int mld_solve_resident(mld_problem_t *p, mld_stats *st)
{
    const int rc = launch(p);
    return rc ? rc : finish(p, st);
}

/* The same solve in two halves, for callers that keep several problems busy: with mld_problem_use_stream every problem owns a HIP stream, a
 * launched solve of one problem runs while another is being prepared or finished, and the workgroups of the next launch move onto the
 * CUs as the stragglers of the previous one retire (bench.py: consecutive, independent scenario sets on two problems). */
int mld_solve_launch(mld_problem_t *p) { return launch(p); }
int mld_solve_finish(mld_problem_t *p, mld_stats *st) { return finish(p, st); }
int mld_problem_use_stream(mld_problem_t *p)
{
    if (!p) { mld_set_error("mld_problem_use_stream: bad handle"); return MLD_ERR_INVALID; }
    if (p->flight != Flight::idle) { mld_set_error("mld_problem_use_stream: a solve is in flight"); return MLD_ERR_INVALID; }
    if (!p->own_stream) { HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking)); p->own_stream = true; }
    return MLD_OK;
}

int mld_download_results(mld_problem_t *p, double *v_out, double *obj_out, int32_t *status_out, double *lower_bound_out,
                         int32_t *nodes_out, int32_t *pivots_out)
{
    if (int rc = entry_guard(p, "mld_download_results", false, "nothing solved")) return rc;
    const size_t b = p->batch;
    if (v_out && p->n) HIP_TRY(hipMemcpy(v_out, p->bat.v, sizeof(double) * b * p->n, hipMemcpyDeviceToHost));
    if (obj_out) HIP_TRY(hipMemcpy(obj_out, p->bat.obj, sizeof(double) * b, hipMemcpyDeviceToHost));
    if (status_out) HIP_TRY(hipMemcpy(status_out, p->bat.status, sizeof(int) * b, hipMemcpyDeviceToHost));
    if (lower_bound_out) HIP_TRY(hipMemcpy(lower_bound_out, p->bat.lbnd, sizeof(double) * b, hipMemcpyDeviceToHost));
    if (nodes_out) HIP_TRY(hipMemcpy(nodes_out, p->bat.nodes, sizeof(int) * b, hipMemcpyDeviceToHost));
    if (pivots_out) HIP_TRY(hipMemcpy(pivots_out, p->bat.pivots, sizeof(int) * b, hipMemcpyDeviceToHost));
    return MLD_OK;
}

int mld_download_telemetry(mld_problem_t *p, int64_t *latency_ns, int64_t *rows_updated, int64_t *row_bytes)
{
    if (int rc = entry_guard(p, "mld_download_telemetry", false, "nothing solved")) return rc;
    const size_t b = p->batch;
    if (latency_ns) {
        std::vector<long long> t(b);
        HIP_TRY(hipMemcpy(t.data(), p->bat.ticks, sizeof(long long) * b, hipMemcpyDeviceToHost));
        int dev = 0, khz = 100000;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
        for (size_t i = 0; i < b; ++i) latency_ns[i] = (int64_t)((double)t[i] * 1.0e6 / (double)khz);
    }
    if (rows_updated) HIP_TRY(hipMemcpy(rows_updated, p->bat.rows, sizeof(long long) * b, hipMemcpyDeviceToHost));
    if (row_bytes) *row_bytes = 8 * SOL_SEC;   /* rows_updated counts update sectors (SOL_SEC doubles) */
    return MLD_OK;
}

/* Post-mortem diagnostics (internal; not part of the public header): every resident workgroup of k_solve writes the instance it is working on and a stage code
 * into 16 ints of HOST memory that is a shared mapping of `path` -- the file survives a GPU fault that takes the process down.  Slot layout per workgroup:
 * [0] instance, [1] stage (1 start, 2 root LP, 10+r / 30+r / 50+r cut round r: Gomory / c-MIR / re-solve, 70 cut loop done, 100 + 10 phase + pass,
 * 400+ leaf, 5000+ flips of the long-step ratio test, 999 instance done), [2] pivots so far, [3] queue position.  path = NULL switches it off. */
int mld_debug_trace(mld_problem_t *p, const char *path)
{
    if (!p) return MLD_ERR_INVALID;
    if (p->h_trace) { (void)hipHostUnregister(p->h_trace); munmap(p->h_trace, p->trace_bytes); p->h_trace = nullptr; p->d_trace = nullptr; }
    if (!path) return MLD_OK;
    const size_t bytes = (size_t)std::max(1, p->n_slots) * 16 * sizeof(int);
    const int fd = open(path, O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (fd < 0 || ftruncate(fd, (off_t)bytes) != 0) { if (fd >= 0) close(fd); mld_set_error("mld_debug_trace: cannot create %s", path); return MLD_ERR_INVALID; }
    void *h = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (h == MAP_FAILED) { mld_set_error("mld_debug_trace: mmap failed"); return MLD_ERR_INVALID; }
    memset(h, 0xff, bytes);
    void *d = nullptr;
    if (hipHostRegister(h, bytes, hipHostRegisterMapped) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        munmap(h, bytes); mld_set_error("mld_debug_trace: hipHostRegister failed"); return MLD_ERR_HIP;
    }
    p->h_trace = h; p->d_trace = (int *)d; p->trace_bytes = bytes;
    return MLD_OK;
}

/* ticks per category summed over the batch (internal diagnostics; not part of the public header) */
int mld_debug_profile(mld_problem_t *p, int64_t out[8])
{
    if (!p || p->batch < 1) return MLD_ERR_INVALID;
    std::vector<long long> t((size_t)p->batch * 8);
    HIP_TRY(hipMemcpy(t.data(), p->bat.prof, sizeof(long long) * t.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; ++k) out[k] = 0;
    for (size_t i = 0; i < (size_t)p->batch; ++i) for (int k = 0; k < 8; ++k) out[k] += t[i * 8 + k];
    return MLD_OK;
}

/* the block reductions of k_solve's selection on n_vec caller-supplied vectors of 512 (value, index) lanes (internal diagnostics; not part of the public
 * header): out_max[4 n_vec] = per vector (block_max1, its DPP version), then per vector (block_min1, its DPP version); out_arg / out_val[2 n_vec] = per
 * vector the arg-max and its value of (block_argmax1, its DPP version) */
int mld_debug_reduce(const double *values, const int32_t *index, int n_vec, double *out_max, int32_t *out_arg, double *out_val)
{
    if (!values || !index || n_vec < 1 || n_vec > 65535 || !out_max || !out_arg || !out_val) { mld_set_error("mld_debug_reduce: bad arguments"); return MLD_ERR_INVALID; }
    if (mld_device_count() <= 0) { mld_set_error("no HIP device"); return MLD_ERR_NO_DEVICE; }
    const size_t len = (size_t)n_vec * SOL_NT;
    DevBuf<double> dv, dmax, dval; DevBuf<int> di, darg;
    HIP_TRY(dv.alloc(len)); HIP_TRY(di.alloc(len)); HIP_TRY(dmax.alloc(4 * (size_t)n_vec)); HIP_TRY(dval.alloc(2 * (size_t)n_vec)); HIP_TRY(darg.alloc(2 * (size_t)n_vec));
    HIP_TRY(hipMemcpy(dv, values, sizeof(double) * len, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(di, index, sizeof(int) * len, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_reduce, dim3(n_vec), dim3(SOL_NT), 0, 0, (const double *)dv, (const int *)di, (double *)dmax, (int *)darg, (double *)dval);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_max, dmax, sizeof(double) * 4 * n_vec, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_arg, darg, sizeof(int) * 2 * n_vec, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_val, dval, sizeof(double) * 2 * n_vec, hipMemcpyDeviceToHost));
    return MLD_OK;
}

/* the row-block sizes of k_solve's row update (internal diagnostics; not part of the public header; no device needed): out[0..3] = rows a wave takes at a
 * time when a chunk has 1, 2, 3, 4 groups of 16 sectors, [4] waves per workgroup, [5] sectors per group, [6] doubles per sector, [7] groups per chunk */
int mld_debug_update_shape(int32_t out[8])
{
    if (!out) { mld_set_error("mld_debug_update_shape: bad arguments"); return MLD_ERR_INVALID; }
    const int32_t v[8] = {s_update_rb(1), s_update_rb(2), s_update_rb(3), s_update_rb(4), SOL_NW, SOL_SPW, SOL_SEC, 4};      // (the templates' own constexpr)
    for (int k = 0; k < 8; ++k) out[k] = v[k];
    return MLD_OK;
}

/* the rows' update of one pivot of k_solve (rowr2 == NULL) or of a fused pair, on a caller-supplied dictionary D (m x ld, row-major; updated in place) (internal
 * diagnostics; not part of the public header): rowr1[n + 1] / colc1[m] the staged (scaled) pivot row and multiplier column of pivot (r1, c1), rowr2 / colc2 /
 * (r2, c2) the second pivot's.  The kernel builds the sector and row lists as the solver does and runs the update: reserved = 0 the default instantiation,
 * MLD_DBG_UPDATE_R7 (and / or MLD_DBG_PIVOT_SYNC_R5) the legacy one.  *rows_updated = the (row, sector) pairs it accounted. */
int mld_debug_update_rows(double *D, int m, int ld, int n, const double *rowr1, const double *colc1, int r1, int c1,
                          const double *rowr2, const double *colc2, int r2, int c2, int reserved, int64_t *rows_updated)
{
    const bool pair = rowr2 != nullptr;
    if (!D || !rowr1 || !colc1 || m < 2 || m > DBG_UPD_MAX || ld < SOL_SEC || ld > DBG_UPD_MAX || ld % SOL_SEC || n < 1 || n >= ld || n + 1 + SOL_SEC <= ld || r1 < 0 || r1 >= m || c1 < 0 || c1 >= n ||
        (pair && (!colc2 || r2 < 0 || r2 >= m || c2 < 0 || c2 >= n)) || (!pair && colc2) || (reserved & ~(MLD_DBG_UPDATE_R7 | MLD_DBG_PIVOT_SYNC_R5))) {
        mld_set_error("mld_debug_update_rows: bad arguments (2 <= m <= %d, ld = n + 1 rounded up to a multiple of %d, at most %d, pivots inside, reserved = bits 26 / 28 only)", DBG_UPD_MAX, SOL_SEC, DBG_UPD_MAX);
        return MLD_ERR_INVALID;
    }
    if (mld_device_count() <= 0) { mld_set_error("no HIP device"); return MLD_ERR_NO_DEVICE; }
    DevBuf<double> dD, dr1, dc1, dr2, dc2; DevBuf<unsigned long long> drows;
    const size_t len = (size_t)m * ld;
    HIP_TRY(dD.alloc(len)); HIP_TRY(dr1.alloc(n + 1)); HIP_TRY(dc1.alloc(m)); HIP_TRY(drows.alloc(1));
    HIP_TRY(hipMemcpy(dD, D, sizeof(double) * len, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dr1, rowr1, sizeof(double) * (n + 1), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dc1, colc1, sizeof(double) * m, hipMemcpyHostToDevice));
    if (pair) {
        HIP_TRY(dr2.alloc(n + 1)); HIP_TRY(dc2.alloc(m));
        HIP_TRY(hipMemcpy(dr2, rowr2, sizeof(double) * (n + 1), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dc2, colc2, sizeof(double) * m, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_debug_update, dim3(1), dim3(SOL_NT), 0, 0, (double *)dD, m, n, ld, (const double *)dr1, (const double *)dc1, r1, c1,
                       pair ? (const double *)dr2 : (const double *)nullptr, pair ? (const double *)dc2 : (const double *)nullptr, r2, c2, pair ? 1 : 0, reserved,
                       (unsigned long long *)drows);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(D, dD, sizeof(double) * len, hipMemcpyDeviceToHost));
    if (rows_updated) { unsigned long long r = 0; HIP_TRY(hipMemcpy(&r, drows, sizeof(r), hipMemcpyDeviceToHost)); *rows_updated = (int64_t)r; }
    return MLD_OK;
}

/* the solver's shape (internal diagnostics; not part of the public header): [0..7] n, m0, mcap, first_cap, ld, mir_cap, lds_bytes, ws_stride;
 * [8..19] the LDS byte offsets (-1: in the slot) lXB, lBasic, lSkip, lAtUp, lNonbasic, lXN, lLo, lHi, lDw, lCost, lMirLine, lMirCache;
 * [20] the LDS budget of the hot arrays, [21] the MLD_SOL_SLOT mask (bit k: SLOT_NAMES[k]), [22] n_slots,
 * [23] lPair: the LDS byte offset of the second pivot's buffers of a fused pair (over lMirCache), or -1: every pivot updates on its own */
int mld_debug_shape(mld_problem_t *p, int64_t out[24])
{
    if (!p || !out) { mld_set_error("mld_debug_shape: bad arguments"); return MLD_ERR_INVALID; }
    const SolverShape &S = p->S;
    const int64_t v[24] = {S.n, S.m0, S.mcap, S.first_cap, S.ld, S.mir_cap, (int64_t)p->lds_bytes, (int64_t)S.ws_stride,
                           S.lXB, S.lBasic, S.lSkip, S.lAtUp, S.lNonbasic, S.lXN, S.lLo, S.lHi, S.lDw, S.lCost, S.lMirLine, S.lMirCache,
                           (int64_t)SOL_LDS_BUDGET, (int64_t)p->slot_mask, p->n_slots, S.lPair};
    for (int k = 0; k < 24; ++k) out[k] = v[k];
    return MLD_OK;
}

/* the MIP start of the resident batch as the next solve would read it (internal diagnostics; not part of the public header): out = batch x n_bin bytes
 * (untouched when there is no start or no binary), *has_warm = 1 when a start is set */
int mld_debug_warm_start(mld_problem_t *p, uint8_t *out, int *has_warm)
{
    if (int rc = entry_guard(p, "mld_debug_warm_start", false, nullptr)) return rc;
    if (!p || p->batch < 1 || !has_warm) { mld_set_error("mld_debug_warm_start: bad arguments / nothing uploaded"); return MLD_ERR_INVALID; }
    *has_warm = p->has_warm ? 1 : 0;
    if (out && p->has_warm && p->nb) HIP_TRY(hipMemcpy(out, p->bat.warm, (size_t)p->batch * p->nb, hipMemcpyDeviceToHost));
    return MLD_OK;
}

int mld_set_warm_start(mld_problem_t *p, const uint8_t *bin_start)
{
    if (int rc = entry_guard(p, "mld_set_warm_start", false, "upload a batch first")) return rc;
    if (!bin_start || p->nb == 0) { p->has_warm = false; return MLD_OK; }
    const size_t tot = (size_t)p->batch * p->nb;
    for (size_t k = 0; k < tot; ++k) if (bin_start[k] > 1 && bin_start[k] != 255) { mld_set_error("mld_set_warm_start: entry %zu is %d (0, 1, or 255 = no start)", k, (int)bin_start[k]); return MLD_ERR_INVALID; }
    HIP_TRY(hipMemcpy(p->bat.warm, bin_start, tot, hipMemcpyHostToDevice));
    p->has_warm = true;
    return MLD_OK;
}

int mld_warm_start_from_previous(mld_problem_t *p, int shift)
{
    if (int rc = entry_guard(p, "mld_warm_start_from_previous", false, nullptr)) return rc;
    if (!p || p->batch < 1 || shift < 0) { mld_set_error("mld_warm_start_from_previous: bad arguments"); return MLD_ERR_INVALID; }
    if (!p->solved) { mld_set_error("mld_warm_start_from_previous: the resident batch has no finished solve (its plan and statuses would be stale or uninitialised)"); return MLD_ERR_INVALID; }
    if (p->nb == 0) { p->has_warm = false; return MLD_OK; }
    const size_t tot = (size_t)p->batch * p->nb;
    hipLaunchKernelGGL(k_warm_from_plan, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, p->stream, p->batch, p->nb, p->nv, p->N, shift, p->d_bins,
                       p->bat.v, (size_t)p->n, p->bat.status, p->bat.obj, p->bat.warm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->has_warm = true;
    return MLD_OK;
}

int mld_set_cutoffs(mld_problem_t *p, const double *cutoff)
{
    if (int rc = entry_guard(p, "mld_set_cutoffs", false, "upload a batch first")) return rc;
    if (!cutoff) { p->has_cutoff = false; return MLD_OK; }
    HIP_TRY(hipMemcpy(p->bat.cutoff, cutoff, sizeof(double) * (size_t)p->batch, hipMemcpyHostToDevice));
    p->has_cutoff = true;
    return MLD_OK;
}

/* In-kernel sub-tree hand-off (DESIGN section 4d; the reference's one backend call per solve, controllers/controller_base.py:509, keeps every core of its
 * machine busy on ONE tree -- this is what lets one solve use more than one compute unit): an instance whose complete depth-first search stops at
 * max_nodes publishes its open nodes as queue entries of the SAME launch; idle workgroups solve them as instances of their own (sub_nodes each,
 * <= max_gen generations, a search with more than max_children open nodes is not split), and the results are merged into the instance on the device.
 * Takes effect with the next mld_upload_batch (the result arrays get room for room_factor x batch items, at least 4096). */
/* build(with_std_constraints=False) / set_constraints(std_evo_constaints=[...]) of the reference (controllers/mpc_controller.py:76-101,
 * controllers/controller_base.py:457-475): the standard block -- rows H_v v <= H_x x + H_w w + H_5 from the batch's own (x0, omega) -- is dropped, only
 * the blocks of mld_upload_constraint_blocks constrain; a row no block covers does not exist for that solve. */
int mld_set_std_block(mld_problem_t *p, int enable)
{
    if (int rc = entry_guard(p, "mld_set_std_block", false, nullptr)) return rc;
    if (!p) { mld_set_error("mld_set_std_block: bad handle"); return MLD_ERR_INVALID; }
    p->std_block = enable != 0;
    return MLD_OK;
}

int mld_set_handoff_policy(mld_problem_t *p, int donate, int rounds)
{
    if (int rc = entry_guard(p, "mld_set_handoff_policy", false, nullptr)) return rc;
    if (!p || donate < 0 || rounds < 0) { mld_set_error("mld_set_handoff_policy: bad arguments"); return MLD_ERR_INVALID; }
    p->ho_donate = std::min(donate, 64); p->ho_rounds = rounds;
    return MLD_OK;
}

int mld_set_handoff(mld_problem_t *p, int enable, int sub_nodes, int max_gen, int max_children, int max_tree, double room_factor)
{
    if (int rc = entry_guard(p, "mld_set_handoff", false, nullptr)) return rc;
    if (!p || sub_nodes < 0 || max_gen < 0 || max_children < 0) { mld_set_error("mld_set_handoff: bad arguments"); return MLD_ERR_INVALID; }
    if (enable && p->nb > 32000) { mld_set_error("mld_set_handoff: too many binaries"); return MLD_ERR_UNSUPPORTED; }
    const bool change = (enable != 0) != (p->ho_enable != 0) || (enable && room_factor > 0.0 && room_factor != p->ho_factor);
    p->ho_enable = enable ? 1 : 0;
    p->ho_sub_nodes = sub_nodes; p->ho_max_gen = max_gen > 0 ? max_gen : 8; p->ho_max_children = max_children > 0 ? max_children : 64;
    if (p->ho_max_gen > 8) p->ho_max_gen = 8;            /* (tree labels: 129^8 < 2^63) */
    if (p->ho_max_children > 64) p->ho_max_children = 64;
    p->ho_max_tree = max_tree > 0 ? max_tree : 160;
    if (room_factor > 0.0) p->ho_factor = room_factor;
    if (change) { free_batch(p); p->batch = 0; }         /* the result arrays are laid out anew by the next upload */
    return MLD_OK;
}

/* diagnostics (internal, not in the public header): per queue entry of the last hand-off solve -- in-kernel ticks, generation, status, root; returns the number of entries */
int mld_debug_entries(mld_problem_t *p, int cap, int64_t *ticks, int32_t *gen, int32_t *status, int32_t *root)
{
    if (!p || !p->ho_ran || !p->bat.ho.tail) return -1;
    int tl = 0;
    if (hipMemcpy(&tl, p->bat.ho.tail, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const int k = std::min(tl, cap);
    (void)hipMemcpy(ticks, p->bat.ticks, sizeof(long long) * k, hipMemcpyDeviceToHost);
    (void)hipMemcpy(status, p->bat.status, sizeof(int) * k, hipMemcpyDeviceToHost);
    if (k > p->batch) {
        (void)hipMemcpy(gen + p->batch, p->bat.ho.item_gen + p->batch, sizeof(int) * (k - p->batch), hipMemcpyDeviceToHost);
        (void)hipMemcpy(root + p->batch, p->bat.ho.item_root + p->batch, sizeof(int) * (k - p->batch), hipMemcpyDeviceToHost);
    }
    for (int i = 0; i < std::min(k, p->batch); ++i) { gen[i] = 0; root[i] = i; }
    return k;
}

/* out[0] items published by the last solve, out[1] reserved, out[2] instances left unfinished although they were split, out[3] entries the arrays have room for */
int mld_handoff_stats(mld_problem_t *p, int64_t out[4])
{
    if (!p || !out) { mld_set_error("mld_handoff_stats: bad arguments"); return MLD_ERR_INVALID; }
    for (int k = 0; k < 4; ++k) out[k] = p->ho_stats[k];
    return MLD_OK;
}

int mld_small_lds_stats(mld_problem_t *p, int64_t out[3])
{
    if (int rc = entry_guard(p, "mld_small_lds_stats", true, nullptr)) return rc;
    if (!p || !out) { mld_set_error("mld_small_lds_stats: bad arguments"); return MLD_ERR_INVALID; }
    out[0] = p->small_ok ? 1 : 0; out[1] = p->small_stats[0]; out[2] = p->small_stats[1];
    return MLD_OK;
}

int mld_record_open_nodes(mld_problem_t *p, int enable)
{
    if (int rc = entry_guard(p, "mld_record_open_nodes", false, nullptr)) return rc;
    if (!p) { mld_set_error("mld_record_open_nodes: bad handle"); return MLD_ERR_INVALID; }
    if (enable && p->n > 32767) { mld_set_error("mld_record_open_nodes: the stacks store variable indices as int16 (n = %d > 32767)", p->n); return MLD_ERR_UNSUPPORTED; }
    p->want_open = enable != 0;
    return MLD_OK;
}

int mld_download_open_nodes(mld_problem_t *p, int32_t *depth_out, int16_t *var_out, uint8_t *val_out, uint8_t *flag_out)
{
    if (int rc = entry_guard(p, "mld_download_open_nodes", false, nullptr)) return rc;
    if (!p || p->batch < 1 || !p->solved || !p->want_open) { mld_set_error("mld_download_open_nodes: no finished solve with mld_record_open_nodes enabled"); return MLD_ERR_INVALID; }
    const size_t b = p->batch, nb = std::max(1, p->nb);
    if (depth_out) HIP_TRY(hipMemcpy(depth_out, p->bat.open_depth, sizeof(int) * b, hipMemcpyDeviceToHost));
    if (var_out) HIP_TRY(hipMemcpy(var_out, p->bat.open_var, sizeof(short) * b * nb, hipMemcpyDeviceToHost));
    if (val_out) HIP_TRY(hipMemcpy(val_out, p->bat.open_val, b * nb, hipMemcpyDeviceToHost));
    if (flag_out) HIP_TRY(hipMemcpy(flag_out, p->bat.open_flag, b * nb, hipMemcpyDeviceToHost));
    return MLD_OK;
}

int mld_stage_inputs(mld_problem_t *p, int n_sets, const double *x0_sets, const double *omega_sets)
{
    if (int rc = entry_guard(p, "mld_stage_inputs", false, "upload a batch first (it fixes the batch size and model_idx)")) return rc;
    if (n_sets < 0 || (n_sets > 0 && ((p->nx && !x0_sets) || (p->nW && !omega_sets)))) { mld_set_error("mld_stage_inputs: bad arguments"); return MLD_ERR_INVALID; }
    p->bat.stage_x0.reset(); p->bat.stage_om.reset();
    p->n_staged = 0; p->staged_batch = 0;
    if (n_sets == 0) return MLD_OK;
    const size_t bx = (size_t)n_sets * p->batch * std::max(1, p->nx), bw = (size_t)n_sets * p->batch * std::max(1, p->nW);
    HIP_TRY(p->bat.stage_x0.alloc(bx));
    HIP_TRY(p->bat.stage_om.alloc(bw));
    if (p->nx) HIP_TRY(hipMemcpy(p->bat.stage_x0, x0_sets, sizeof(double) * (size_t)n_sets * p->batch * p->nx, hipMemcpyHostToDevice));
    if (p->nW) HIP_TRY(hipMemcpy(p->bat.stage_om, omega_sets, sizeof(double) * (size_t)n_sets * p->batch * p->nW, hipMemcpyHostToDevice));
    p->n_staged = n_sets; p->staged_batch = p->batch;
    return MLD_OK;
}

int mld_select_inputs(mld_problem_t *p, int set)
{
    if (int rc = entry_guard(p, "mld_select_inputs", false, nullptr)) return rc;
    if (!p || p->batch < 1 || p->staged_batch != p->batch || set < 0 || set >= p->n_staged) { mld_set_error("mld_select_inputs: set %d not staged for this batch", set); return MLD_ERR_INVALID; }
    if (p->nx) HIP_TRY(hipMemcpyAsync(p->bat.x0, p->bat.stage_x0 + (size_t)set * p->batch * p->nx, sizeof(double) * (size_t)p->batch * p->nx, hipMemcpyDeviceToDevice, p->stream));
    if (p->nW) HIP_TRY(hipMemcpyAsync(p->bat.omega, p->bat.stage_om + (size_t)set * p->batch * p->nW, sizeof(double) * (size_t)p->batch * p->nW, hipMemcpyDeviceToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));   /* the other entry points copy on the legacy stream, which does not order against a non-blocking one */
    inputs_replaced(p);
    return MLD_OK;
}

int mld_download_inputs(mld_problem_t *p, double *x0, double *omega)
{
    if (int rc = entry_guard(p, "mld_download_inputs", false, "nothing uploaded")) return rc;
    if (x0 && p->nx) HIP_TRY(hipMemcpy(x0, p->bat.x0, sizeof(double) * (size_t)p->batch * p->nx, hipMemcpyDeviceToHost));
    if (omega && p->nW) HIP_TRY(hipMemcpy(omega, p->bat.omega, sizeof(double) * (size_t)p->batch * p->nW, hipMemcpyDeviceToHost));
    return MLD_OK;
}

int mld_solve_batch(mld_problem_t *p, int batch, const int32_t *model_idx, const double *x0, const double *omega,
                    const uint8_t *fixed_bin, double *v_out, double *obj_out, int32_t *status_out,
                    double *lower_bound_out, mld_stats *stats_out)
{
    int rc = mld_upload_batch(p, batch, model_idx, x0, omega, fixed_bin);
    if (rc) return rc;
    if ((rc = mld_solve_resident(p, stats_out))) return rc;
    return mld_download_results(p, v_out, obj_out, status_out, lower_bound_out, nullptr, nullptr);
}

int mld_rhs_batch(mld_problem_t *p, int batch, int scenarios, const int32_t *model_idx, const double *x0,
                  const double *omega, double *h_out)
{
    if (!p || batch < 1 || scenarios < 1 || !h_out) { mld_set_error("mld_rhs_batch: bad arguments"); return MLD_ERR_INVALID; }
    if ((p->nx && !x0) || (p->nW && !omega)) { mld_set_error("mld_rhs_batch: x0/omega required"); return MLD_ERR_INVALID; }
    if (model_idx) for (int k = 0; k < batch; ++k) if (model_idx[k] < 0 || model_idx[k] >= p->n_models) { mld_set_error("model_idx[%d]=%d out of range", k, model_idx[k]); return MLD_ERR_INVALID; }
    mld_model *m = p->model;
    int rc;
    if (m->cond_N != p->N && (rc = condense_model_device(m, p->N, nullptr, 0))) return rc;
    /* temporaries of this call: released on every return path (HIP_TRY returns early) */
    DevBuf<int> d_idx, d_perm; DevBuf<double> d_x, d_w, d_h; DevBuf<RhsGroup> d_groups;
    const size_t b = batch;
    if (model_idx) { HIP_TRY(d_idx.alloc(b)); HIP_TRY(hipMemcpy(d_idx, model_idx, sizeof(int) * b, hipMemcpyHostToDevice)); }
    HIP_TRY(d_x.alloc(b * std::max(1, p->nx)));
    HIP_TRY(d_w.alloc(b * scenarios * std::max(1, p->nW)));
    HIP_TRY(d_h.alloc(b * std::max(1, p->m0)));
    if (p->nx) HIP_TRY(hipMemcpy(d_x, x0, sizeof(double) * b * p->nx, hipMemcpyHostToDevice));
    if (p->nW) HIP_TRY(hipMemcpy(d_w, omega, sizeof(double) * b * scenarios * p->nW, hipMemcpyHostToDevice));
    if (p->m0 && scenarios == 1 && rhs_mfma_fits(p->nx, p->nW) && !(p->opts.reserved & MLD_DBG_GEMM_VALU)) {
        std::vector<int> perm; std::vector<RhsGroup> groups;
        build_rhs_groups(model_idx, batch, p->n_models, perm, groups);
        if (!perm.empty()) { HIP_TRY(d_perm.alloc(perm.size())); HIP_TRY(hipMemcpy(d_perm, perm.data(), sizeof(int) * perm.size(), hipMemcpyHostToDevice)); }
        HIP_TRY(d_groups.alloc(groups.size()));
        HIP_TRY(hipMemcpy(d_groups, groups.data(), sizeof(RhsGroup) * groups.size(), hipMemcpyHostToDevice));
        launch_rhs_mfma((p->opts.flags & MLD_F32) != 0, (int)groups.size(), p->m0, p->nx, p->nW, m->d_out[O_HX], m->d_out[O_HW], m->d_out[O_H5],
                        (const double *)nullptr, d_groups, d_perm, d_x, d_w, d_h);
    } else if (p->m0) {
        hipLaunchKernelGGL(k_rhs, dim3(batch), dim3(256), 0, 0, p->m0, p->nx, p->nW, m->d_out[O_HX], m->d_out[O_HW], m->d_out[O_H5],
                           (const double *)nullptr, d_idx, d_x, d_w, d_h, scenarios);
    }
    if (p->m0) {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(h_out, d_h, sizeof(double) * b * p->m0, hipMemcpyDeviceToHost));
    }
    return MLD_OK;
}

} // extern "C"
