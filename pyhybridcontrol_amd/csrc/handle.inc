// The problem handle: its device buffers, the LDS placement ladder, batch (re)allocation, and the host helpers every entry point is written from.
/* buffers of the uploaded batch (ensure_batch, mld_upload_batch, mld_upload_constraint_blocks, mld_stage_inputs): released together when the
 * batch is laid out anew.  Inputs have one entry per instance, results one per queue entry (instances, then the items of the in-kernel hand-off). */
struct BatchBufs {
    DevBuf<int> model_idx; DevBuf<double> x0, omega, hs, qs_inst, rconst;
    DevBuf<double> x0b, omegab; DevBuf<int> skipped;     /* spare input buffers and device counter of mld_advance_batch (the counter: also the hand-off merge's) */
    DevBuf<unsigned char> warm; DevBuf<int> order;       /* MIP start (mld_set_warm_start); longest-first work-queue order learnt from the previous solve */
    DevBuf<unsigned char> fixed; DevBuf<double> cutoff, v, obj, lbnd;
    DevBuf<int> status, nodes, pivots, cuts, refac; DevBuf<long long> ticks, rows, prof;
    DevBuf<int> open_depth; DevBuf<short> open_var; DevBuf<unsigned char> open_val, open_flag;   /* open-node stacks (mld_download_open_nodes) */
    DevBuf<double> stage_x0, stage_om;                   /* resident input sets (mld_stage_inputs) */
    DevBuf<int> perm; DevBuf<RhsGroup> groups;           /* instances grouped by model for the MFMA right-hand sides (K3) */
    DevBuf<double> xcols, xcols_x; DevBuf<int> xrows;    /* extra constraint blocks; the state every extra column was generated with (explicit x_k) */
    DevBuf<double> sim_tmp;                              /* scratch of k_sim_step where its staging does not fit LDS: in_cap x (nomega + ny), on first use */
    DevBuf<double> icost, qs_inst_t;                     /* per-instance linear cost (mld_upload_instance_cost): batch x ic_ld, unscaled, pulled back to v
                                                            [then cx | cw | c0]; qs_inst under the Toeplitz-compatible column scales (k_lp_lds, on first use) */
    struct Handoff {      /* in-kernel sub-tree hand-off queue: allocated only while mld_set_handoff has it on */
        DevBuf<int> tail, finished, item_src, item_root, item_gen, item_ready, item_children; DevBuf<long long> item_label;
        DevBuf<unsigned long long> mg_best, mg_lbopen, mg_label; DevBuf<int> mg_open;   /* merge accumulators per root */
        DevBuf<int> tree_count, tree_dead;                /* items published per tree / tree given up */
    } ho;
};

/* what mld_solve_finish has to do: nothing launched; a dense solve queued on the stream; or an LDS-path solve that ran to completion in the
 * launch (the fall-back needs its statuses on the host), whose finish only reports */
enum class Flight : unsigned char { idle, queued, lds_done };

/* A resident array of start offsets into the profile library, (batch, cols, pf_groups) on the device; cols is 1 where the array has no column axis.  It
 * belongs to a batch SIZE (batch, 0 = none resident); per group the largest resident start is kept on the host, so that a call with start == NULL is
 * checked against the window rule without reading the device. */
struct PfStarts {
    DevBuf<long long> d; int batch = 0, cols = 0; std::vector<long long> gmax;
    void reset() { d.reset(); batch = cols = 0; }
};
/* the starts of a call become the resident ones (once the stream has taken them) */
static void set_starts(PfStarts &r, DevBuf<long long> &&d, int batch, int cols, const std::vector<long long> &gmax)
{
    r.d = std::move(d); r.batch = batch; r.cols = cols; r.gmax = gmax;
}

struct mld_problem {
    mld_model *model = nullptr;                 // caller's (original) model: used by mld_rhs_batch
    std::unique_ptr<mld_model> tight;           // internal copy with tightened rows, condensed on device
    mld_opts opts{};
    int N_p = 0, N = 0, n = 0, m0 = 0, nb = 0, nx = 0, nW = 0, nv = 0, n_models = 0;
    void *h_trace = nullptr; int *d_trace = nullptr; size_t trace_bytes = 0;   /* mld_debug_trace: file-backed host buffer the kernel writes its stage markers into */
    int mir_cap = 0;            /* integer entries of the widest scaled original row over all models, rounded up to 8 (k_solve's compact c-MIR lines) */
    SolverShape S{};
    unsigned slot_mask = 0;     /* MLD_SOL_SLOT at creation: the hot arrays build_shape kept in the slot (bit k: SLOT_NAMES[k]) */
    // per-model device arrays
    DevBuf<double> d_Gp;        /* d_Gs with columns in dictionary (position-major) order: coalesced dictionary reset */
    DevBuf<double> d_actmax;    /* n_models x m0: largest row activity under the model's bounds (s_mark_dead) */
    /* sparse copies of the scaled rows for the per-instance presolve (s_presolve): by row and by column, nnz_cap entries per model */
    DevBuf<int> d_csr_ptr, d_csc_ptr; DevBuf<unsigned short> d_csr_col, d_csc_row; DevBuf<double> d_csr_val, d_csc_val; int nnz_cap = 0;
    DevBuf<double> d_Gs, d_rs, d_cs, d_qs, d_lb, d_ub, d_cx, d_cw, d_c0, d_q0;
    DevBuf<unsigned char> d_is_int;
    DevBuf<int> d_bins, d_colperm, d_binpos;   /* d_binpos: position of a structural among the binaries, -1 for continuous entries (in-kernel hand-off) */
    // quadratic cost (K4)
    DevBuf<double> d_P, d_Qx, d_Qw, d_Ps, d_Wx, d_Wy;
    bool has_quad = false;
    // workspace
    DevBuf<unsigned char> d_ws; DevBuf<int> d_counter;
    int n_slots = 0;
    size_t lds_bytes = 0;
    // batch buffers, and what they hold: every per-entry result array has batch_cap entries, the inputs in_cap
    BatchBufs bat;
    int batch = 0, batch_cap = 0, in_cap = 0;
    bool has_fixed = false, has_midx = false, has_warm = false;
    bool solved = false;        /* the resident batch has a finished solve (mld_advance_batch / mld_warm_start_from_previous need one) */
    bool advanced = false;      /* mld_advance_batch has applied that solve's plan: the next advance needs the next solve */
    bool has_cutoff = false, want_open = false;    /* objective cutoffs (mld_set_cutoffs); record the open-node stacks (mld_record_open_nodes) */
    int n_staged = 0, staged_batch = 0, n_groups = 0, n_xcols = 0, order_batch = 0; size_t xcols_cap = 0; bool has_xcols_x = false;
    int ic_ld = 0;              /* row length of bat.icost: 0 = no per-instance cost resident, n = weights on v only, n + nx + nW + 1 = with the constant's maps */
    DevBuf<double> d_gather; size_t gather_cap = 0;   /* send + receive buffers of mld_gather_results */
    /* LDS-resident LP path (k_lp_lds): Toeplitz-compatible scaling of the tightened model */
    bool lp_ok = false, all_fixed = false; LpShape LS{}; size_t lp_lds_bytes = 0; int lp_slots = 0;
    DevBuf<double> d_blk_t, d_rs_t, d_cs_t, d_lb_t, d_ub_t, d_qs_t;
    /* small-problem path (k_small_milp, MLD_SMALL_LDS): decided once in mld_problem_create; the device counter of the declined instances; what the last solve did */
    bool small_ok = false; SmShape SS{}; size_t small_lds_bytes = 0; int small_slots = 0; DevBuf<int> d_declined;
    long long small_stats[2] = {};   /* last solve: instances answered in LDS, instances the dense kernel re-solved */
    hipEvent_t ev[3] = {}; bool ev_ok = false; DevBuf<long long> d_statbuf;
    hipStream_t stream = 0; bool own_stream = false; Flight flight = Flight::idle;   /* stream of the solve path (0 = the legacy stream); a launched, not yet finished solve */
    bool std_block = true;      /* the standard constraint block (right-hand side from the batch's own omega) is part of the problem (mld_set_std_block) */
    /* in-kernel sub-tree hand-off (mld_set_handoff) */
    int ho_enable = 0, ho_sub_nodes = 0, ho_max_gen = 0, ho_max_children = 0; double ho_factor = 2.0; bool ho_ran = false;
    int ho_max_tree = 160, ho_donate = 0, ho_rounds = 0;   /* items per tree; shallow open nodes handed off per node-limit, times */
    /* resident disturbance profiles (mld_upload_profiles): owned by the problem, not by the batch -- free_batch leaves them alone; and the resident starts
     * of the forecast windows, of the constraint columns' windows and of the REALISED series (mld_sim_step_batch, MLD_SIM_ACTUAL), each an array of its own */
    DevBuf<double> pf_lib; long long pf_len = 0; int pf_groups = 0; std::vector<int> pf_width; DevBuf<PfChan> pf_chan;
    PfStarts pf_forecast, pf_columns, pf_actual;
    /* resident price profiles (mld_upload_prices): a flat library of its own, owned by the problem like the one above; a series is row-major (time, pr_chan).
     * pr_cost: the resident starts of the cost windows (mld_instance_cost_from_prices).  pr_tab: the tables of mld_set_price_cost, [a_v | sum_v | a_y], each
     * (n_models, pr_chan, nv / nv / ny), zeros where the caller gave none; pr_ay: a_y was given (the cost then needs the pull-back).  sc_tab: the stage weights
     * of mld_set_stage_cost, [w_v | w_y], (n_models, pr_chan, nv / ny).  The tables are shaped by pr_chan: a library with another n_chan drops them */
    DevBuf<double> pr_lib; long long pr_len = 0; int pr_chan = 0; PfStarts pr_cost;
    DevBuf<double> pr_tab, sc_tab; bool pr_tab_on = false, pr_ay = false, sc_on = false;
    /* resident simulation log (mld_sim_log_begin): `cap` records of the resident batch, one array per field, each (cap, batch, width).  It belongs to the
     * resident batch: mld_upload_batch discards it */
    struct SimLog {
        DevBuf<double> x, v, y, om, x_k1, vio, obj, lb; DevBuf<unsigned char> cons; DevBuf<int> row, status, nodes;
        DevBuf<int> aux;        /* (cap, batch) resolver statuses of the records mld_sim_step_resolve wrote, -2 elsewhere: allocated by the first such step that logs */
        DevBuf<int> src;        /* (cap, batch) u_source of the records mld_sim_step_fallback wrote, -2 elsewhere: allocated by the first such step that logs */
        DevBuf<int> pick;       /* (cap, batch) the candidate the records of mld_sim_step_selected applied (-1: another source), -2 elsewhere: allocated likewise */
        /* stage cost (mld_sim_log_cost_begin), armed while `cost` is allocated: cost (cap, batch) and price (cap, batch, pr_chan) beside the records, the
         * running total and the count of stepped records per instance, the starts into the price library and the largest of them */
        DevBuf<double> cost, price, total; DevBuf<int> steps; DevBuf<long long> cstart; long long cstart_max = 0;
        void disarm() { cost.reset(); price.reset(); total.reset(); steps.reset(); cstart.reset(); cstart_max = 0; }
        int cap = 0, count = 0;
    } slog;
    /* mld_sim_step_resolve: batch_gen numbers the uploads of all handles (inputs_new_batch), so that a resolver handle can tell whether its resident batch
     * is still the one laid out for the stepped handle's -- it remembers that handle's number and its own at the time (0 = never laid out) */
    unsigned long long batch_gen = 0, aux_src_gen = 0, aux_own_gen = 0;
    /* rule-based feedback policy (mld_upload_policy): the tables (n_models, nu, nx + 5) -- per channel [sel | on_at | off_at | u_on | u_off | mode] -- on
     * the device and on the host, owned by the problem like the profile library.  The resident u_prev (batch, nu) belongs to ONE upload of a batch: it is
     * valid while pol_state_gen == batch_gen, and laid out as the reset state (u_off on the ruled channels) by the first call that needs it after that */
    DevBuf<double> pol_tab, pol_uprev; std::vector<double> pol_host; bool pol_on = false, pol_all_ruled = false; unsigned long long pol_state_gen = 0;
    /* plan memory (mld_plan_memory, mld_sim_step_fallback): mem_u (batch, N, nu) the u of the last usable plan of every instance, mem_age (batch) the advancing
     * steps since (-1 nothing remembered, N exhausted).  Like the policy state it belongs to ONE upload of a batch (mem_batch_gen == batch_gen), and it is valid
     * only along an unbroken chain of advancing fallback steps: chain_gen counts every event that replaces x0 or advances the inputs (inputs_replaced,
     * inputs_advanced_by_plan); the fallback step adopts the count after its own advance (mem_chain).  Where either number has moved on, the first call that
     * needs the memory empties it (plan_memory_ready) */
    DevBuf<double> mem_u; DevBuf<int> mem_age; bool mem_on = false; unsigned long long mem_batch_gen = 0, mem_chain = 0, chain_gen = 0;
    /* device completion of declined rollout trajectories (mld_set_rollout_completion): the sticky mode of this (stepped) handle, and what the last call of the
     * rollout family did -- rounds, trajectories finished on the device, dense solves, trajectories left declined (mld_rollout_completion_stats) */
    int ro_mode = 0; long long ro_stats[4] = {};
    /* kept selection (mld_keep_selection, mld_set_selection, mld_sim_step_selected): what the last successful mld_rollout_select[_policy] chose -- choice and
     * policy (batch), u (batch, K, nu) -- or what the caller set.  Stamped with batch_gen and chain_gen: valid while both are unchanged, the plan memory's rule,
     * so a new forecast, a solve and a new cost keep it and an upload, new inputs and every advance end it.  sel_keep: the sticky switch of the select calls */
    struct Selection {
        DevBuf<int> choice, policy; DevBuf<double> u; int K = 0, batch = 0; bool has = false; unsigned long long batch_gen = 0, chain = 0;
    } sel;
    bool sel_keep = false;
    long long ho_stats[4] = {};  /* last solve: items published, trees split, trees left unfinished, entries the queue had no room for (always 0: such trees stay unfinished) */
};

/* ---- What a change of the inputs leaves of the state that belonged to the previous ones (tests/test_gpu_input_state.py).  The extra constraint blocks
 * (n_xcols), the MIP start (has_warm) and the cutoffs belong to ONE set of inputs; `solved` says that the result arrays hold a finished solve of the resident
 * batch (mld_advance_batch, mld_warm_start_from_previous, mld_predict_batch ... need one), `advanced` that its plan has been applied: the next advance needs
 * the next solve, and the plan belongs to inputs that are gone. ---- */
/* new inputs for the same batch (mld_select_inputs): the blocks belonged to the previous inputs, so did the start and the cutoffs; there is no plan */
static void inputs_replaced(mld_problem *p) { p->n_xcols = 0; p->has_warm = false; p->solved = false; p->advanced = false; p->has_cutoff = false; ++p->chain_gen; }
/* a new batch (mld_upload_batch): nothing of the previous one stays -- the blocks, a simulation log and a per-instance cost belong to one upload */
static std::atomic<unsigned long long> g_batch_gen{0};
static void inputs_new_batch(mld_problem *p)
{
    inputs_replaced(p);
    p->batch_gen = ++g_batch_gen;
    if (p->slog.cap) p->slog = mld_problem::SimLog();
    if (p->ic_ld) { p->bat.icost.reset(); p->bat.qs_inst_t.reset(); p->ic_ld = 0; }
}
/* inputs advanced by the resident plan (mld_advance_batch, mld_sim_step_batch): the blocks belonged to the previous step's data, a start belongs to one set
 * of inputs (mld_warm_start_from_previous builds the next one from the plan, so the batch stays `solved`); the plan has been applied */
static void inputs_advanced_by_plan(mld_problem *p) { p->n_xcols = 0; p->has_warm = false; p->has_cutoff = false; p->advanced = true; ++p->chain_gen; }
/* inputs advanced by the caller's v0 (mld_sim_step_batch): the resident plan had no part in them -- new inputs, as after mld_select_inputs */
static void inputs_advanced_by_caller(mld_problem *p) { inputs_replaced(p); }
/* the forecast replaced (mld_forecast_from_profiles): new inputs, as mld_select_inputs -- except after an advance, where the new forecast completes the
 * step: the blocks are gone already, and plan and start stay.  x0 and the clock stay either way, so a plan memory stays valid (chain_gen is kept) */
static void forecast_replaced(mld_problem *p) { if (!p->advanced) { const unsigned long long chain = p->chain_gen; inputs_replaced(p); p->chain_gen = chain; } }

/* the resident starts point into ONE library: they go with it */
static void reset_profile_starts(mld_problem *p) { p->pf_forecast.reset(); p->pf_columns.reset(); p->pf_actual.reset(); }

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* mld_opts.time_limit (seconds) in ticks of the device's constant wall clock (wall_clock64: 100 MHz on gfx950) */
static long long time_limit_ticks(double seconds)
{
    if (!(seconds > 0.0)) return 0;
    int dev = 0, khz = 100000;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
    const double t = seconds * 1.0e3 * (double)khz;
    return t >= 9.0e18 ? (long long)9.0e18 : (long long)std::max(1.0, t);
}

/* MLD_SOL_SLOT (diagnostics and tests): a comma list of the hot arrays that stay in the slot even where they would fit in LDS, or "all"; the rest of the
 * placement ladder runs as before.  Read when the problem is created (build_shape); an unknown name is an error, so that a typo cannot test the default. */
static const char *const SLOT_NAMES[] = {"xb", "basic", "skip", "atup", "nonbasic", "xn", "lohi", "dw", "cost", "mirline", "mircache"};
enum { SLOT_N = (int)(sizeof(SLOT_NAMES) / sizeof(SLOT_NAMES[0])) };

static int sol_slot_mask(unsigned *mask)
{
    *mask = 0;
    const char *env = getenv("MLD_SOL_SLOT");
    if (!env) return MLD_OK;
    const std::string all(env);
    size_t b = 0;
    while (b <= all.size()) {
        size_t e = all.find(',', b);
        if (e == std::string::npos) e = all.size();
        const std::string name = all.substr(b, e - b);
        int k = 0;
        if (name == "all") *mask |= (1u << SLOT_N) - 1u;
        else if (!name.empty()) {
            while (k < SLOT_N && name != SLOT_NAMES[k]) ++k;
            if (k == SLOT_N) { mld_set_error("MLD_SOL_SLOT: unknown array '%s' (xb, basic, skip, atup, nonbasic, xn, lohi, dw, cost, mirline, mircache, all)", name.c_str()); return MLD_ERR_INVALID; }
            *mask |= 1u << k;
        }
        b = e + 1;
    }
    return MLD_OK;
}

static int build_shape(mld_problem *p)
{
    unsigned slot = 0;
    if (int rc = sol_slot_mask(&slot)) return rc;
    p->slot_mask = slot;
    SolverShape &S = p->S;
    const mld_opts &o = p->opts;
    /* cut rows: max_cuts for the root cut loop + S_RESTART_ROWS (0) that only the root restart may use (k_solve: more cut rounds at the root once an incumbent leaves a
     * small gap; the first loop needs its max_cuts -- capping it lower to make room measured +37 % row updates on the steady-state instances) */
    const int restart_rows = (o.max_cuts > 0 && o.cut_rounds > 0) ? S_RESTART_ROWS : 0;
    S.n = p->n; S.m0 = p->m0; S.mcap = p->m0 + o.max_cuts + restart_rows; S.first_cap = p->m0 + o.max_cuts; S.ld = (p->n + 1 + 7) & ~7;   /* rows start on 64-byte sectors */
    S.ntot = p->n + S.mcap;
    S.nb = p->nb; S.nx = p->nx; S.nW = p->nW; S.N = p->N; S.nv = p->nv;
    S.max_cuts = o.max_cuts; S.cuts_per_round = o.cuts_per_round; S.cut_rounds = o.cut_rounds;
    S.max_nodes = o.max_nodes; S.max_pivots = o.max_pivots; S.gap_abs = o.gap_abs; S.gap_rel = o.gap_rel;
    S.debug = o.reserved;
    S.presolve = (o.presolve & 4) && p->m0 < 65536 && p->n < 65536 ? 1 : 0;
    S.time_ticks = time_limit_ticks(o.time_limit);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t r = off; off = align_up(off + bytes, 256); return r; };
    const size_t n = S.n, mc = S.mcap, nt = S.ntot, nb = std::max(1, S.nb);
    S.oD = take(sizeof(double) * (mc + 1) * S.ld);
    S.oGc = take(sizeof(double) * std::max<size_t>(1, o.max_cuts + restart_rows) * n);
    S.oHc = take(sizeof(double) * std::max<size_t>(1, o.max_cuts + restart_rows));
    S.oLo = take(sizeof(double) * nt); S.oHi = take(sizeof(double) * nt);
    S.oXB = take(sizeof(double) * mc); S.oXN = take(sizeof(double) * n);
    S.oBasic = take(sizeof(int) * mc); S.oNonbasic = take(sizeof(int) * n); S.oWhere = take(sizeof(int) * nt);
    S.oAtUp = take(n); S.oSkip = take(mc);
    S.oTmpX = take(sizeof(double) * n); S.oG = take(sizeof(double) * n); S.oAx = take(sizeof(double) * n);
    S.oRootLo = take(sizeof(double) * n); S.oRootHi = take(sizeof(double) * n);
    S.oStkJ = take(sizeof(int) * (nb + 2)); S.oStkF = take(nb + 2); S.oStkS = take(nb + 2);
    S.oSvJ = take(sizeof(int) * (nb + 2)); S.oSvLo = take(sizeof(double) * (nb + 2)); S.oSvHi = take(sizeof(double) * (nb + 2));
    S.oKey = take(sizeof(double) * std::max<size_t>(std::max<size_t>(mc, nb + 2), 64)); S.oXo = take(sizeof(double) * n);
    S.oY = take(sizeof(double) * 33 * n); S.oPY = take(sizeof(double) * 33 * n);
    S.oHm = take(sizeof(double) * 32 * 32); S.oCm = take(sizeof(double) * 32); S.oWm = take(sizeof(double) * 32);
    S.oGcost = take(sizeof(double) * n); S.oVcur = take(sizeof(double) * n); S.oPv = take(sizeof(double) * n);
    S.oXroot = take(sizeof(double) * (nb + 2)); S.oFxLo = take(sizeof(double) * (nb + 2)); S.oFxHi = take(sizeof(double) * (nb + 2));
    S.oFxJ = take(sizeof(int) * (nb + 2));
    S.oMirEff = take(sizeof(double) * std::max<size_t>(1, S.m0)); S.oMirDelta = take(sizeof(double) * std::max<size_t>(1, S.m0));
    S.oMirCache = take(sizeof(double) * SOL_NW * 2 * n);
    S.oDw = take(sizeof(double) * mc);
    S.oLive = take(sizeof(unsigned short) * std::max<size_t>(8, S.m0));
    S.oMq = take(sizeof(double) * SD_MQ_DOUBLES);      /* work arrays of the master QP (simplicial decomposition) */
    S.oClo = take(sizeof(double) * n); S.oChi = take(sizeof(double) * n);      /* bounds the cut builders may use for the continuous structurals (s_presolve) */
    S.oStkV = take(nb + 2);                             /* the search path's values while a stopped search closes its open siblings (in-kernel hand-off) */
    S.mir_per_round = o.mir_per_round;
    S.ws_stride = align_up(off, 4096);
    S.seccap = (int)std::max<size_t>(std::max<size_t>(mc + 8, n + 8), (n + SOL_SEC) / SOL_SEC + 8);      /* (also the list of the columns the long-step ratio test flips: up to n) */
    p->lds_bytes = sizeof(double) * (n + 2 + mc + 2 + n + 2) + sizeof(unsigned short) * ((size_t)S.seccap + mc + 8 + 8);
    /* hot per-basis state moves from the slot into LDS while it fits (one workgroup per CU: 160 KB LDS) */
    size_t loff = align_up(p->lds_bytes, 16);
#ifndef SOL_LDS_BUDGET
#define SOL_LDS_BUDGET ((SOL_WPE >= 4 ? 78 : 144) * 1024)
#endif
    const size_t budget = SOL_LDS_BUDGET;
    /* k: the array's bit in the MLD_SOL_SLOT mask (SLOT_NAMES) */
    auto ltake = [&](size_t bytes, int k) -> int { const size_t b = align_up(bytes, 16); if ((slot >> k & 1u) || loff + b > budget) return -1; const size_t r = loff; loff += b; return (int)r; };
    S.lXB = ltake(sizeof(double) * mc, 0); S.lBasic = ltake(sizeof(int) * mc, 1); S.lSkip = ltake(mc, 2);
    S.lAtUp = ltake(n, 3); S.lNonbasic = ltake(sizeof(int) * n, 4); S.lXN = ltake(sizeof(double) * n, 5);
    S.lLo = ltake(sizeof(double) * nt, 6); S.lHi = S.lLo >= 0 ? ltake(sizeof(double) * nt, 6) : -1;
    S.lDw = ltake(sizeof(double) * mc, 7);
    S.lCost = ltake(sizeof(double) * (n + 1), 8);                     /* the reduced-cost row: read by every ratio test, updated by every pivot */
    S.mir_cap = p->mir_cap; S.lMirLine = -1;
    if (p->mir_cap > 0 && p->mir_cap < n) S.lMirLine = ltake(sizeof(double) * SOL_NW * 2 * p->mir_cap, 9);  /* compact lines of the c-MIR scoring (a row's free binaries) */
    S.lMirCache = ltake(sizeof(double) * SOL_NW * 2 * n, 10);                                              /* full-width lines (Gomory rounds): LDS while it fits */
    /* Buffers of the second pivot of a fused pair (s_pivot_pair): row, multiplier column, union lists, sector flags.  They need no bytes of their own: the per-wave
     * lines of lMirCache are scratch of the cut rounds and dead while the dual simplex runs, so the pair's buffers lie over them when every hot array is in LDS. */
    {
        const bool all_lds = S.lXB >= 0 && S.lXN >= 0 && S.lLo >= 0 && S.lHi >= 0 && S.lBasic >= 0 && S.lNonbasic >= 0 && S.lAtUp >= 0 && S.lSkip >= 0 && S.lDw >= 0 && S.lCost >= 0;
        S.lPair = (all_lds && S.lMirCache >= 0 && pair_lds_bytes(S.n, S.mcap) <= sizeof(double) * SOL_NW * 2 * n) ? S.lMirCache : -1;
    }
    p->lds_bytes = loff;
    return MLD_OK;
}

/* a host array to a buffer of its own size (an empty array leaves the buffer empty) */
template <typename T> static int upload(DevBuf<T> &dst, const std::vector<T> &src)
{
    if (src.empty()) { dst.reset(); return MLD_OK; }
    HIP_TRY(dst.alloc(src.size()));
    HIP_TRY(hipMemcpy(dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    return MLD_OK;
}

static void free_batch(mld_problem *p)
{
    p->bat = BatchBufs();
    if (p->slog.cap) p->slog = mld_problem::SimLog();
    p->n_groups = 0; p->has_warm = false; p->solved = false; p->advanced = false; p->has_cutoff = false;
    p->n_staged = 0; p->staged_batch = 0; p->n_xcols = 0; p->xcols_cap = 0; p->has_xcols_x = false;
    p->order_batch = 0; p->in_cap = 0; p->batch_cap = 0; p->ic_ld = 0;
}

/* entries the per-entry arrays need for a batch: with the in-kernel hand-off the queue has room for ho_factor x batch items (at least 4096) behind the instances */
static size_t entry_cap_for(const mld_problem *p, int batch)
{
    if (!p->ho_enable) return (size_t)batch;
    return (size_t)batch + std::max<size_t>(4096, (size_t)(p->ho_factor * (double)batch));
}

static int ensure_batch(mld_problem *p, int batch)
{
    const size_t cap = entry_cap_for(p, batch);
    if (batch <= p->in_cap && cap <= (size_t)p->batch_cap) return MLD_OK;
    free_batch(p);
    const size_t b = batch;
    /* inputs: one per instance */
    HIP_TRY(p->bat.model_idx.alloc(b));
    HIP_TRY(p->bat.x0.alloc(b * std::max(1, p->nx)));
    HIP_TRY(p->bat.omega.alloc(b * std::max(1, p->nW)));
    HIP_TRY(p->bat.x0b.alloc(b * std::max(1, p->nx)));
    HIP_TRY(p->bat.omegab.alloc(b * std::max(1, p->nW)));
    HIP_TRY(p->bat.warm.alloc(b * std::max(1, p->nb)));
    HIP_TRY(p->bat.skipped.alloc(1));
    HIP_TRY(p->bat.hs.alloc(b * std::max(1, p->m0)));
    HIP_TRY(p->bat.qs_inst.alloc(b * std::max(1, p->n)));
    HIP_TRY(p->bat.rconst.alloc(b));
    HIP_TRY(p->bat.order.alloc(b));
    /* per entry (instances, then the items of the in-kernel hand-off) */
    HIP_TRY(p->bat.fixed.alloc(cap * std::max(1, p->nb)));
    HIP_TRY(p->bat.cutoff.alloc(cap));
    HIP_TRY(p->bat.open_depth.alloc(cap));
    HIP_TRY(p->bat.open_var.alloc(cap * std::max(1, p->nb)));
    HIP_TRY(p->bat.open_val.alloc(cap * std::max(1, p->nb)));
    HIP_TRY(p->bat.open_flag.alloc(cap * std::max(1, p->nb)));
    HIP_TRY(p->bat.v.alloc(cap * std::max(1, p->n)));
    HIP_TRY(p->bat.obj.alloc(cap));
    HIP_TRY(p->bat.lbnd.alloc(cap));
    HIP_TRY(p->bat.status.alloc(cap)); HIP_TRY(p->bat.nodes.alloc(cap));
    HIP_TRY(p->bat.pivots.alloc(cap)); HIP_TRY(p->bat.cuts.alloc(cap));
    HIP_TRY(p->bat.refac.alloc(cap));
    HIP_TRY(hipMemset(p->bat.status, 0, sizeof(int) * cap));      /* (ADVICE r3: a reallocation must not leave stale statuses for mld_warm_start_from_previous) */
    HIP_TRY(p->bat.ticks.alloc(cap)); HIP_TRY(p->bat.rows.alloc(cap));
    HIP_TRY(p->bat.prof.alloc(cap * 8));
    if (p->ho_enable) {
        HIP_TRY(p->bat.ho.tail.alloc(1)); HIP_TRY(p->bat.ho.finished.alloc(1));
        HIP_TRY(p->bat.ho.item_src.alloc(cap)); HIP_TRY(p->bat.ho.item_root.alloc(cap));
        HIP_TRY(p->bat.ho.item_gen.alloc(cap)); HIP_TRY(p->bat.ho.item_ready.alloc(cap));
        HIP_TRY(p->bat.ho.item_children.alloc(cap)); HIP_TRY(p->bat.ho.item_label.alloc(cap));
        HIP_TRY(p->bat.ho.mg_best.alloc(b)); HIP_TRY(p->bat.ho.mg_lbopen.alloc(b));
        HIP_TRY(p->bat.ho.mg_label.alloc(b)); HIP_TRY(p->bat.ho.mg_open.alloc(b));
        HIP_TRY(p->bat.ho.tree_count.alloc(b * 9)); HIP_TRY(p->bat.ho.tree_dead.alloc(b));
    }
    p->order_batch = 0;
    p->in_cap = batch;
    p->batch_cap = (int)cap;
    return MLD_OK;
}

// ---- the parts an entry point is written from ----------------------------------------------------------------------------------------------------
/* The checks an entry point begins with, in this order: a HIP device (need_device); no launched solve that has not been finished -- it owns the problem's
 * buffers until mld_solve_finish --; a resident batch (no_batch: the text after "who: " it is refused with, NULL = not tested here). */
static int entry_guard(const mld_problem *p, const char *who, bool need_device, const char *no_batch)
{
    if (need_device && mld_device_count() <= 0) { mld_set_error("no HIP device (libmldgpu has no CPU fallback)"); return MLD_ERR_NO_DEVICE; }
    if (p && p->flight != Flight::idle) { mld_set_error("%s: a launched solve has not been finished (mld_solve_finish)", who); return MLD_ERR_INVALID; }
    if (no_batch && (!p || p->batch < 1)) { mld_set_error("%s: %s", who, no_batch); return MLD_ERR_INVALID; }
    return MLD_OK;
}

/* Queue, then always wait.  `queue` puts the copies and kernels of a call on the stream and returns its error; nothing of the caller's and no temporary of
 * the call may go before the stream has drained, on EVERY path -- a queueing that failed half-way included.  The queue's error comes first, the wait's
 * second.  wait = false (a step of mld_sim_step_batch that reports nothing to the host) leaves a call that queued without an error asynchronous. */
template <typename Queue> static int queue_and_wait(hipStream_t sq, Queue &&queue, bool wait = true)
{
    const int rc = queue();
    if (!rc && !wait) return MLD_OK;
    const hipError_t es = hipStreamSynchronize(sq);
    if (rc) return rc;
    HIP_TRY(es);
    return MLD_OK;
}

/* What a policy entry point adds to the body it shares with its open-loop neighbour (rollout_impl): the inputs before step 0 (NULL: the resident policy
 * state) and where the switch counts go */
struct PolicyCall { const double *u_prev; int32_t *switches_out; };

/* One policy's tables tested and laid out in the kernels' rows -- per model and channel [sel (nx) | on_at | off_at | u_on | u_off | mode] -- into tab
 * (M nu (nx + 5) doubles): the one copy of what mld_upload_policy and mld_rollout_select_policy refuse.  table < 0: mld_upload_policy's own arguments and
 * messages; table >= 0: table `table` of the pol_* arrays of a selection, named in every message, where a passed-through channel is refused too (a policy
 * candidate rules every channel).  all_ruled (or NULL): whether every channel is ruled. */
static int policy_table_fill(const char *who, int table, int M, int nx, int nu, const double *sel, const double *on_at, const double *off_at, const double *u_on,
                             const double *u_off, const int32_t *mode, double *tab, bool *all_ruled)
{
    const int row = nx + POL_TAIL;
    const char *pre = table < 0 ? "" : "pol_";
    char at[32] = "";
    if (table >= 0) snprintf(at, sizeof at, "table %d, ", table);
    bool all = true;
    for (int m = 0; m < M; ++m)
        for (int j = 0; j < nu; ++j) {
            const size_t c = (size_t)m * nu + j;
            double *t = tab + c * row;
            for (int i = 0; i < nx; ++i) {
                t[i] = sel[c * nx + i];
                if (!std::isfinite(t[i])) { mld_set_error("%s: %ssel of %smodel %d, channel %d, state %d is not finite (%g)", who, pre, at, m, j, i, t[i]); return MLD_ERR_INVALID; }
            }
            const double vals[4] = {on_at[c], off_at[c], u_on[c], u_off[c]};
            static const char *const names[4] = {"on_at", "off_at", "u_on", "u_off"};
            for (int k = 0; k < 4; ++k) {
                if (!std::isfinite(vals[k])) { mld_set_error("%s: %s%s of %smodel %d, channel %d is not finite (%g)", who, pre, names[k], at, m, j, vals[k]); return MLD_ERR_INVALID; }
                t[nx + k] = vals[k];
            }
            if (on_at[c] > off_at[c]) { mld_set_error("%s: %son_at > %soff_at for %smodel %d, channel %d (%g > %g): the band between the thresholds would be empty", who, pre, pre, at, m, j, on_at[c], off_at[c]); return MLD_ERR_INVALID; }
            if (mode[c] != 0 && mode[c] != 1) { mld_set_error("%s: %smode of %smodel %d, channel %d is %d (0 = passed through, 1 = ruled)", who, pre, at, m, j, (int)mode[c]); return MLD_ERR_INVALID; }
            if (table >= 0 && mode[c] == 0) {
                mld_set_error("%s: pol_mode of table %d, model %d, channel %d is 0 (passed through): a policy candidate rules every channel -- a candidate that rules some channels and takes the plan for the others is not built",
                              who, table, m, j);
                return MLD_ERR_INVALID;
            }
            t[nx + POL_MODE] = (double)mode[c];
            all = all && mode[c] == 1;
        }
    if (all_ruled) *all_ruled = all;
    return MLD_OK;
}

/* What mld_rollout_kpi adds to the same body: the KPI tables of mld_sim_log_summary (each (n_models, n_kpi, width) or NULL), the starts into the price
 * library (batch, or NULL) and where the statistics go: sum, min, max, min_step, max_step, n_above, n_changes (batch, S, n_kpi), n_vio (batch, S); any NULL */
struct KpiCall {
    int n_kpi;
    const double *tab[5];      /* w_x, w_v, w_y, w_omega, w_xk1 */
    const int32_t *price_chan; const double *thresh; double vio_tol; const int64_t *price_start;
    double *sum, *min, *max; int32_t *min_step, *max_step, *n_above, *n_changes, *n_vio;
};

/* Where the results of a rollout go on the host, in the order of the entry points' arguments: per trajectory and step x (K + 1 states), v, y, cons_vio,
 * cons_row; per trajectory cost, mu_total, worst_vio, worst_step, steps_done, end_status; stats[4].  Any may be NULL: not asked for */
struct RolloutOut {
    double *x, *v, *y, *cons_vio; int32_t *cons_row;
    double *cost, *mu_total, *worst_vio; int32_t *worst_step, *steps_done, *end_status;
    int64_t *stats;
};

/* What mld_rollout_risk adds to the same body: the columns (G) as (src, q) with their exceedance levels (G, or NULL = +inf), the levels alpha (L), and where
 * the statistics across the realisations go: mean, min, max, min_c, max_c, n_exceed (batch, G), quantile, quantile_c, cvar_hi, cvar_lo (batch, G, L),
 * counts (batch, 4); any NULL */
struct RiskCall {
    int G; const int32_t *col_src, *col_q; const double *level;
    int L; const double *alpha;
    double *mean, *min, *max; int32_t *min_c, *max_c, *n_exceed;
    double *quantile; int32_t *quantile_c; double *cvar_hi, *cvar_lo;
    int32_t *counts;
};

/* What mld_rollout_select adds to the same body (always beside a RiskCall, never a PolicyCall): P candidates per instance -- candidate 0 the resident plan
 * where plan_first is set, the others u_cand (batch, P - plan_first, K, nu) --, the rule (plan_select.inc: objective, constraints, min_complete) and where the
 * choice goes: choice, score, n_admissible (batch), admissible (batch, P), u_choice (batch, K, nu), u0_choice (batch, nu); any NULL.  Every per-trajectory
 * output of the call is (batch, P, S, ...), every risk output (batch, P, G[, L]), counts (batch, P, 4). */
struct SelectCall {
    int P, plan_first; const double *u_cand;
    int obj_col, obj_kind, obj_level;
    int n_cons; const int32_t *cons_col, *cons_kind, *cons_level; const double *cons_bound;
    int min_complete;
    int32_t *choice; double *score; int32_t *n_admissible; uint8_t *admissible; double *u_choice, *u0_choice;
    /* mld_rollout_select_policy: the last T of the P candidates are rule policies in closed loop (T == 0: mld_rollout_select's call) -- their tables
     * pol_sel (T, n_models, nu, nx), pol_on_at, pol_off_at, pol_u_on, pol_u_off, pol_mode (T, n_models, nu), the inputs before step 0 (batch, nu; NULL: the
     * resident policy state) and where the switch counts go (batch, P, S; NULL); u_cand is (batch, P - plan_first - T, K, nu) */
    int T; const double *pol_sel, *pol_on_at, *pol_off_at, *pol_u_on, *pol_u_off; const int32_t *pol_mode; const double *u_prev; int32_t *switches_out;
};

/* What mld_warm_start_from_rollout adds to the same body: the rows that have a start keep it (MLD_START_KEEP), and where the source per instance (batch, or
 * NULL) and the counts [trajectories, written, kept, none] (or NULL) go */
struct StartCall { bool keep; int32_t *source_out; int64_t *stats; };

/* The resident policy state of THIS upload of the batch: if there is none yet (or it belonged to an earlier upload), the reset state -- every ruled channel
 * at its model's u_off, the reference's first step, which has no previous record (theromstat_control.py:57: `u_k_neg1 == 1` is false); a passed-through
 * channel at 0.  Host-synchronous on the legacy stream, before the caller queues anything. */
static int policy_state_ready(mld_problem *p, const char *who)
{
    if (!p->pol_on) { mld_set_error("%s: no policy uploaded (mld_upload_policy)", who); return MLD_ERR_INVALID; }
    if (p->pol_uprev && p->pol_state_gen == p->batch_gen) return MLD_OK;
    const int batch = p->batch, nu = p->model->dims.nu, row = p->model->dims.nx + POL_TAIL;
    std::vector<int32_t> midx;
    if (p->has_midx) { midx.resize(batch); HIP_TRY(hipMemcpy(midx.data(), p->bat.model_idx, sizeof(int) * batch, hipMemcpyDeviceToHost)); }
    std::vector<double> init((size_t)batch * nu);
    for (int b = 0; b < batch; ++b)
        for (int j = 0; j < nu; ++j) {
            const double *t = p->pol_host.data() + ((size_t)(p->has_midx ? midx[b] : 0) * nu + j) * row + (row - POL_TAIL);
            init[(size_t)b * nu + j] = t[POL_MODE] != 0.0 ? t[POL_U_OFF] : 0.0;
        }
    p->pol_state_gen = 0;
    HIP_TRY(p->pol_uprev.alloc(std::max<size_t>(1, init.size())));
    if (!init.empty()) HIP_TRY(hipMemcpy(p->pol_uprev, init.data(), sizeof(double) * init.size(), hipMemcpyHostToDevice));
    p->pol_state_gen = p->batch_gen;
    return MLD_OK;
}

/* The plan memory of THIS upload of the batch, along an unbroken chain of advancing fallback steps: where the batch has been uploaded anew the buffers are
 * laid out for its size, and where anything else has replaced x0 or advanced the inputs since the memory was last valid, every age goes back to -1
 * (nothing remembered).  Host-synchronous, before the caller queues anything. */
static int plan_memory_ready(mld_problem *p, const char *who)
{
    if (!p->mem_on) { mld_set_error("%s: no plan memory enabled (mld_plan_memory)", who); return MLD_ERR_INVALID; }
    const bool same_batch = p->mem_u && p->mem_batch_gen == p->batch_gen;
    if (same_batch && p->mem_chain == p->chain_gen) return MLD_OK;
    const size_t batch = (size_t)p->batch, len = batch * p->N * p->model->dims.nu;
    const hipStream_t sq = p->stream;
    DevBuf<double> u; DevBuf<int> age;
    if (!same_batch) { HIP_TRY(u.alloc(std::max<size_t>(1, len))); HIP_TRY(age.alloc(batch)); }
    auto fill = [&]() -> int {
        if (!same_batch) HIP_TRY(hipMemsetAsync(u, 0, sizeof(double) * std::max<size_t>(1, len), sq));
        HIP_TRY(hipMemsetAsync(same_batch ? p->mem_age.get() : age.get(), 0xff, sizeof(int) * batch, sq));      /* every byte 0xff: -1 */
        return MLD_OK;
    };
    if (int rc = queue_and_wait(sq, fill)) return rc;
    if (!same_batch) { p->mem_u = std::move(u); p->mem_age = std::move(age); }
    p->mem_batch_gen = p->batch_gen; p->mem_chain = p->chain_gen;
    return MLD_OK;
}

/* col_rows of n_cols extra columns (NULL = every column covers all rows): the leading rows a column constrains, 0 .. m0.  who: prefix of the message, or NULL */
static int check_col_rows(const mld_problem *p, const char *who, int n_cols, const int32_t *col_rows)
{
    if (col_rows) for (int c = 0; c < n_cols; ++c) if (col_rows[c] < 0 || col_rows[c] > p->m0) {
        mld_set_error("%s%scol_rows[%d]=%d outside [0,%d]", who ? who : "", who ? ": " : "", c, col_rows[c], p->m0); return MLD_ERR_INVALID;
    }
    return MLD_OK;
}

/* Room for n_cols extra constraint columns of the resident batch (mld_upload_constraint_blocks_x, mld_constraint_blocks_from_profiles): bat.xcols grown to
 * batch x n_cols x nW, bat.xrows where the columns come with col_rows, bat.xcols_x where they come with the state they were generated with (has_xcols_x).
 * The resident blocks are gone from the first line on; the caller fills the buffers and sets n_xcols when everything has arrived. */
static int stage_xcols(mld_problem *p, int n_cols, bool with_rows, bool with_x)
{
    p->n_xcols = 0;
    const size_t need = (size_t)p->batch * n_cols * p->nW;
    if (need > p->xcols_cap) {
        p->xcols_cap = 0;
        HIP_TRY(p->bat.xcols.alloc(need));
        p->xcols_cap = need;
    }
    p->bat.xrows.reset();
    if (with_rows) HIP_TRY(p->bat.xrows.alloc(n_cols));
    p->has_xcols_x = false;
    if (with_x) HIP_TRY(p->bat.xcols_x.alloc((size_t)p->batch * n_cols * p->nx));
    p->has_xcols_x = with_x;
    return MLD_OK;
}

/* the stacked state and output maps of the tightened model, per family [v, x, w, 5], as k_inst_pullback and k_trajectory read them (a family without rows: null) */
static PbMaps pullback_maps(const mld_problem *p)
{
    const mld_model *t = p->tight.get();
    const int NX = p->N * p->model->dims.nx, NY = p->N * p->model->dims.ny;
    PbMaps mp;
    const int oW[4] = {O_GamV, O_PhiX, O_GamW, O_Gam5}, oY[4] = {O_LV, O_LX, O_LW, O_L5};
    for (int f = 0; f < 4; ++f) {
        mp.W[f] = NX ? t->d_out[oW[f]].get() : nullptr; mp.sW[f] = t->lay.out_size[oW[f]];
        mp.Y[f] = NY ? t->d_out[oY[f]].get() : nullptr; mp.sY[f] = t->lay.out_size[oY[f]];
    }
    return mp;
}

/* The per-instance part of the cost (quadratic atoms on x / y, mld_upload_instance_cost) at the CURRENT inputs, staged / advanced ones included:
 * qs = cs (q0 + q_b + Qx x0 + Qw omega) and rconst = e'We of the quadratic atoms + cx_b' x0 + cw_b' omega + c0_b.  cs: the column scales -- d_cs for the
 * solve path, ones for mld_evaluate_batch, which writes into buffers of its own; cs_t / qs_t (or null): a second copy of qs under the Toeplitz-compatible
 * scales (k_lp_lds; never with a quadratic cost).  For a problem with has_quad || ic_ld. */
static int launch_instance_cost(mld_problem *p, const double *cs, double *qs, double *rconst, const double *cs_t, double *qs_t)
{
    const hipStream_t sq = p->stream;
    const int batch = p->batch, n = p->n, nx = p->nx, nW = p->nW;
    const size_t tot = (size_t)batch * n;
    const int *midx = p->has_midx ? p->bat.model_idx.get() : nullptr;
    HIP_TRY(hipMemsetAsync(rconst, 0, sizeof(double) * batch, sq));
    if (p->has_quad) {
        const mld_model *t = p->tight.get();
        const int NX = p->N * p->model->dims.nx, NY = p->N * p->model->dims.ny;
        hipLaunchKernelGGL(k_qinst, dim3(batch), dim3(256), 0, sq, n, nx, nW, p->d_q0, p->d_Qx, p->d_Qw, cs, midx, p->bat.x0, p->bat.omega, qs,
                           p->ic_ld ? p->bat.icost.get() : nullptr, p->ic_ld);
        if (p->d_Wx && NX) hipLaunchKernelGGL(k_quad_const, dim3(batch), dim3(256), sizeof(double) * NX, sq, NX, nx, nW, t->d_out[O_PhiX], t->lay.out_size[O_PhiX],
                                              t->d_out[O_GamW], t->lay.out_size[O_GamW], t->d_out[O_Gam5], t->lay.out_size[O_Gam5], p->d_Wx, midx, p->bat.x0, p->bat.omega, rconst);
        if (p->d_Wy && NY) hipLaunchKernelGGL(k_quad_const, dim3(batch), dim3(256), sizeof(double) * NY, sq, NY, nx, nW, t->d_out[O_LX], t->lay.out_size[O_LX],
                                              t->d_out[O_LW], t->lay.out_size[O_LW], t->d_out[O_L5], t->lay.out_size[O_L5], p->d_Wy, midx, p->bat.x0, p->bat.omega, rconst);
    } else if (tot)
        hipLaunchKernelGGL(k_inst_cost, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, sq, tot, n, p->ic_ld, p->d_q0, cs, cs_t, midx, p->bat.icost, qs, qs_t);
    if (p->ic_ld > n)
        hipLaunchKernelGGL(k_inst_const, dim3((batch + 3) / 4), dim3(256), 0, sq, batch, n, nx, nW, p->ic_ld, p->bat.icost, p->bat.x0, p->bat.omega, rconst);
    return MLD_OK;
}

// ---- resident profiles: the window rule on the host ------------------------------------------------------------------------------------------------------
/* the words by which the messages of the window rule differ: a window of N steps behind a start (forecast, columns), ONE element behind an actual start,
 * or a price window behind a start into the price library */
struct PfWords { const char *start, *window; bool column; const char *lib; };
static const PfWords PF_WINDOW = {"start", "window", true, "library"}, PF_ELEMENT = {"actual start", "element", false, "library"},
                     PF_PRICE = {"price start", "price window", false, "price library"}, PF_PRICE_ELEMENT = {"price start", "price", false, "price library"};

/* the library a start array points into, as the window rule sees it: its length and its groups' widths (the disturbance library: one group per fused device;
 * the price library: ONE group of width n_chan) */
struct PfLibView { long long len; int groups; const int *width; };
static PfLibView profile_lib(const mld_problem *p) { return PfLibView{p->pf_len, p->pf_groups, p->pf_width.data()}; }
static PfLibView price_lib(const mld_problem *p) { return PfLibView{p->pr_len, 1, &p->pr_chan}; }

/* what the three consumers share: a library and a step the window rule can be tested with */
static int profile_ready(const mld_problem *p, const char *who, int step)
{
    if (!p->pf_len) { mld_set_error("%s: no profile library resident (mld_upload_profiles)", who); return MLD_ERR_INVALID; }
    if (step < 0 || step > INT_MAX - p->N) { mld_set_error("%s: step = %d (must be >= 0)", who, step); return MLD_ERR_INVALID; }
    return MLD_OK;
}

/* every start of a (batch, n_cols, n_groups) array against the window rule for `len` steps (N for a window, 1 for an element); the first offender is named;
 * gmax: per group the largest start */
static int check_starts(const PfLibView &L, const char *who, const PfWords &w, const int64_t *start, int batch, int n_cols, int step, int len, std::vector<long long> &gmax)
{
    const int G = L.groups;
    gmax.assign(G, 0);
    const int64_t *s = start;
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < n_cols; ++c)
            for (int g = 0; g < G; ++g, ++s) {
                if (!profile_start_ok(*s, L.len, step, len, L.width[g])) {
                    char col[32] = "";
                    if (w.column) snprintf(col, sizeof(col), " column %d,", c);
                    mld_set_error("%s: %s %lld of instance %d,%s group %d (width %d) at step %d: the %s [%lld, %lld) leaves the %s of %lld doubles",
                                  who, w.start, (long long)*s, b, col, g, L.width[g], step, w.window, (long long)*s + (long long)step * L.width[g],
                                  (long long)*s + ((long long)step + len) * L.width[g], w.lib, L.len);
                    return MLD_ERR_INVALID;
                }
                gmax[g] = std::max<long long>(gmax[g], *s);
            }
    return MLD_OK;
}
static int profile_check_starts(const mld_problem *p, const char *who, const PfWords &w, const int64_t *start, int batch, int n_cols, int step, int len, std::vector<long long> &gmax)
{
    return check_starts(profile_lib(p), who, w, start, batch, n_cols, step, len, gmax);
}

/* resident starts under another step: the remembered maxima decide (the smallest start was >= 0 when the array was uploaded) */
static int check_resident(const PfLibView &L, const char *who, const PfWords &w, const std::vector<long long> &gmax, int step, int len)
{
    for (int g = 0; g < L.groups; ++g)
        if (!profile_start_ok(gmax[g], L.len, step, len, L.width[g])) {
            mld_set_error("%s: step %d moves the largest resident %s of group %d (%lld, width %d) past the end of the %s: the %s would end at %lld of %lld doubles",
                          who, step, w.start, g, gmax[g], L.width[g], w.lib, w.window, gmax[g] + ((long long)step + len) * L.width[g], L.len);
            return MLD_ERR_INVALID;
        }
    return MLD_OK;
}
static int profile_check_resident(const mld_problem *p, const char *who, const PfWords &w, const std::vector<long long> &gmax, int step, int len)
{
    return check_resident(profile_lib(p), who, w, gmax, step, len);
}
