// Problem creation, cost (K4) and options.
static int set_cost_impl(mld_problem *p, const mld_cost *cost)
{
    const int n = p->n, M = p->n_models, nx = p->nx, nW = p->nW;
    const int NX = p->N * p->model->dims.nx, NY = p->N * p->model->dims.ny;
    const mld_model *t = p->tight.get();
    /* Everything runs on the problem's own stream and ends with a wait on THAT stream: a caller that updates the cost of one problem every step
     * (the reference rebuilds its objective with the new prices before every solve, micro_grid_control_simulation.py:197-198,229) must not stall
     * the solve another problem has in flight.  A purely linear cost on v (lin_v only: the bench's q_z / q_mu atoms) needs no temporary and no
     * host round trip: upload, scale on the device. */
    const hipStream_t sq = p->stream;
    // q0 = lin_v + Gamma_v' lin_x + L_v' lin_y ; cx = Phi' lin_x + L_x' lin_y ; cw = Gamma_w' lin_x + L_w' lin_y ; c0 = ...
    HIP_TRY(hipMemsetAsync(p->d_q0, 0, sizeof(double) * n * M, sq));
    HIP_TRY(hipMemsetAsync(p->d_cx, 0, sizeof(double) * std::max(1, nx) * M, sq));
    HIP_TRY(hipMemsetAsync(p->d_cw, 0, sizeof(double) * std::max(1, nW) * M, sq));
    HIP_TRY(hipMemsetAsync(p->d_c0, 0, sizeof(double) * M, sq));
    if (cost && cost->lin_v) HIP_TRY(hipMemcpyAsync(p->d_q0, cost->lin_v, sizeof(double) * n * M, hipMemcpyHostToDevice, sq));
    auto pull = [&](const double *hw, int len, int oV, int oX, int oW, int o5) -> int {
        if (!hw || len == 0) return MLD_OK;
        DevBuf<double> d_w;      /* (released on every return path) */
        HIP_TRY(d_w.alloc((size_t)len * M));
        HIP_TRY(hipMemcpyAsync(d_w, hw, sizeof(double) * len * M, hipMemcpyHostToDevice, sq));
        const dim3 blk(256);
        if (t->d_out[oV]) hipLaunchKernelGGL(k_pullback, dim3((n + 255) / 256, M), blk, 0, sq, len, n, t->d_out[oV], t->lay.out_size[oV], d_w, (size_t)len, p->d_q0, (size_t)n, 1);
        if (nx && t->d_out[oX]) hipLaunchKernelGGL(k_pullback, dim3((nx + 255) / 256, M), blk, 0, sq, len, nx, t->d_out[oX], t->lay.out_size[oX], d_w, (size_t)len, p->d_cx, (size_t)nx, 1);
        if (nW && t->d_out[oW]) hipLaunchKernelGGL(k_pullback, dim3((nW + 255) / 256, M), blk, 0, sq, len, nW, t->d_out[oW], t->lay.out_size[oW], d_w, (size_t)len, p->d_cw, (size_t)nW, 1);
        if (t->d_out[o5]) hipLaunchKernelGGL(k_pullback, dim3(1, M), blk, 0, sq, len, 1, t->d_out[o5], t->lay.out_size[o5], d_w, (size_t)len, p->d_c0, (size_t)1, 1);
        HIP_TRY(hipStreamSynchronize(sq));      /* (the temporary is released when this scope ends) */
        return MLD_OK;
    };
    int rc;
    if (cost) {
        if ((rc = pull(cost->lin_x, NX, O_GamV, O_PhiX, O_GamW, O_Gam5))) return rc;
        if ((rc = pull(cost->lin_y, NY, O_LV, O_LX, O_LW, O_L5))) return rc;
    }
    // quadratic part (assembled for mld_cost_assemble; the MILP solver rejects it)
    p->has_quad = cost && (cost->quad_v || cost->quad_x || cost->quad_y);
    p->d_P.reset(); p->d_Qx.reset(); p->d_Qw.reset(); p->d_Ps.reset(); p->d_Wx.reset(); p->d_Wy.reset();
    if (p->has_quad) {
        HIP_TRY(p->d_P.alloc((size_t)n * n * M));
        HIP_TRY(hipMemset(p->d_P, 0, sizeof(double) * (size_t)n * n * M));
        if (nx) { HIP_TRY(p->d_Qx.alloc((size_t)n * nx * M)); HIP_TRY(hipMemset(p->d_Qx, 0, sizeof(double) * (size_t)n * nx * M)); }
        if (nW) { HIP_TRY(p->d_Qw.alloc((size_t)n * nW * M)); HIP_TRY(hipMemset(p->d_Qw, 0, sizeof(double) * (size_t)n * nW * M)); }
        if (cost->quad_v) {
            DevBuf<double> d_W, d_Ws;
            HIP_TRY(d_W.alloc((size_t)n * n * M)); HIP_TRY(d_Ws.alloc((size_t)n * n * M));
            HIP_TRY(hipMemcpyAsync(d_W, cost->quad_v, sizeof(double) * (size_t)n * n * M, hipMemcpyHostToDevice, sq));
            hipLaunchKernelGGL(k_symmetrize, dim3(((size_t)n * n + 255) / 256, M), dim3(256), 0, sq, n, d_W, d_Ws, (size_t)n * n);
            HIP_TRY(hipMemcpyAsync(p->d_P, d_Ws, sizeof(double) * (size_t)n * n * M, hipMemcpyDeviceToDevice, sq));
            HIP_TRY(hipStreamSynchronize(sq));
        }
        auto quad = [&](const double *hW, int len, int oV, int oX, int oW, int o5, DevBuf<double> &keepW) -> int {
            if (!hW || len == 0) return MLD_OK;
            const size_t ll = (size_t)len * len;
            DevBuf<double> d_W, d_Ws, d_T;
            HIP_TRY(d_W.alloc(ll * M)); HIP_TRY(d_Ws.alloc(ll * M));
            const size_t tcols = (size_t)std::max(std::max(n, nx), std::max(nW, 1));     /* d_T also holds the len x nx and len x nW products */
            HIP_TRY(d_T.alloc((size_t)len * tcols * M));
            HIP_TRY(hipMemcpyAsync(d_W, hW, sizeof(double) * ll * M, hipMemcpyHostToDevice, sq));
            hipLaunchKernelGGL(k_symmetrize, dim3((ll + 255) / 256, M), dim3(256), 0, sq, len, d_W, d_Ws, ll);
            // T = Ws * Mv (len x n) ; P += Mv' T ; Qx += (Ws Mx)' ... computed as Mv' (Ws Mx)
            const dim3 blk(256);
            auto gemm = [&](int Mm, int Nn, int K, int tA, const double *A, size_t sA, const double *Bp, size_t sB, double *Cp, size_t sC, double beta) {
                if (p->opts.reserved & MLD_DBG_GEMM_VALU) hipLaunchKernelGGL(k_gemm, dim3((Nn + 15) / 16, (Mm + 15) / 16, M), blk, 0, sq, Mm, Nn, K, tA, A, sA, Bp, sB, Cp, sC, 1.0, beta);
                else if (p->opts.flags & MLD_F32) hipLaunchKernelGGL(k_gemm_mfma<true>, dim3((Nn + GM_T - 1) / GM_T, (Mm + GM_T - 1) / GM_T, M), blk, 0, sq, Mm, Nn, K, tA, A, sA, Bp, sB, Cp, sC, 1.0, beta);
                else hipLaunchKernelGGL(k_gemm_mfma<false>, dim3((Nn + GM_T - 1) / GM_T, (Mm + GM_T - 1) / GM_T, M), blk, 0, sq, Mm, Nn, K, tA, A, sA, Bp, sB, Cp, sC, 1.0, beta);
            };
            if (t->d_out[oV]) {
                gemm(len, n, len, 0, d_Ws, ll, t->d_out[oV], t->lay.out_size[oV], d_T, (size_t)len * tcols, 0.0);
                gemm(n, n, len, 1, t->d_out[oV], t->lay.out_size[oV], d_T, (size_t)len * tcols, p->d_P, (size_t)n * n, 1.0);
                if (nx && t->d_out[oX]) {
                    gemm(len, nx, len, 0, d_Ws, ll, t->d_out[oX], t->lay.out_size[oX], d_T, (size_t)len * tcols, 0.0);
                    gemm(n, nx, len, 1, t->d_out[oV], t->lay.out_size[oV], d_T, (size_t)len * tcols, p->d_Qx, (size_t)n * nx, 1.0);
                }
                if (nW && t->d_out[oW]) {
                    gemm(len, nW, len, 0, d_Ws, ll, t->d_out[oW], t->lay.out_size[oW], d_T, (size_t)len * tcols, 0.0);
                    gemm(n, nW, len, 1, t->d_out[oV], t->lay.out_size[oV], d_T, (size_t)len * tcols, p->d_Qw, (size_t)n * nW, 1.0);
                }
                if (t->d_out[o5]) {
                    gemm(len, 1, len, 0, d_Ws, ll, t->d_out[o5], t->lay.out_size[o5], d_T, (size_t)len * tcols, 0.0);
                    gemm(n, 1, len, 1, t->d_out[oV], t->lay.out_size[oV], d_T, (size_t)len * tcols, p->d_q0, (size_t)n, 1.0);
                }
            }
            HIP_TRY(hipStreamSynchronize(sq));
            keepW = std::move(d_W);      // un-symmetrised weight, kept for the objective constant e'We
            return MLD_OK;
        };
        if ((rc = quad(cost->quad_x, NX, O_GamV, O_PhiX, O_GamW, O_Gam5, p->d_Wx))) return rc;
        if ((rc = quad(cost->quad_y, NY, O_LV, O_LX, O_LW, O_L5, p->d_Wy))) return rc;
        HIP_TRY(p->d_Ps.alloc((size_t)n * n * M));
        hipLaunchKernelGGL(k_scale_P, dim3(((size_t)n * n + 255) / 256, M), dim3(256), 0, sq, n, p->d_P, p->d_cs, p->d_Ps);
    }
    // scaled cost for the solver: qs = q0 .* cs (and with the Toeplitz-compatible column scales for the LDS-resident LP path)
    const size_t tot = (size_t)n * M;
    if (tot) {
        hipLaunchKernelGGL(k_scale_vec, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, sq, tot, p->d_q0, p->d_cs, p->d_qs);
        if (p->lp_ok) hipLaunchKernelGGL(k_scale_vec, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, sq, tot, p->d_q0, p->d_cs_t, p->d_qs_t);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sq));
    return MLD_OK;
}

extern "C" {

/* sizeof(mld_opts) of THIS build: a binding compiled against another layout of the struct must not call mld_problem_create (checked by the Python loader) */
int mld_opts_size(void) { return (int)sizeof(mld_opts); }

int mld_opts_default(mld_opts *o)
{
    if (!o) return MLD_ERR_INVALID;
    o->gap_abs = 1e-9; o->gap_rel = 0.0; o->max_nodes = 100000; o->max_pivots = 50000; o->cut_rounds = -1;
    o->cuts_per_round = -1; o->max_cuts = -1; o->presolve = 6; o->n_slots = 0; o->mir_per_round = -1; o->flags = 0; o->reserved = 0; o->time_limit = 0.0;
    return MLD_OK;
}

/* the device buffers release themselves with the handle; the solve path's stream is drained first (a queued kernel may still use them and the trace) */
int mld_problem_destroy(mld_problem_t *p)
{
    if (!p) return MLD_OK;
    (void)hipStreamSynchronize(p->stream);
    if (p->ev_ok) { (void)hipEventDestroy(p->ev[0]); (void)hipEventDestroy(p->ev[1]); (void)hipEventDestroy(p->ev[2]); }
    if (p->own_stream) (void)hipStreamDestroy(p->stream);
    if (p->h_trace) { (void)hipHostUnregister(p->h_trace); munmap(p->h_trace, p->trace_bytes); }
    delete p;
    return MLD_OK;
}

int mld_problem_create(mld_problem_t **out, mld_model_t *model, int N_p, int N_tilde, const mld_cost *cost,
                       const mld_opts *opts)
{
    if (!out || !model || N_tilde < 1) { mld_set_error("mld_problem_create: bad arguments"); return MLD_ERR_INVALID; }
    std::unique_ptr<mld_problem, int (*)(mld_problem_t *)> p(new mld_problem(), mld_problem_destroy);      /* (every error return releases it) */
    p->model = model;
    if (opts) p->opts = *opts; else mld_opts_default(&p->opts);
    const mld_dims &d = model->dims;
    p->N_p = N_p; p->N = N_tilde; p->nv = model->nv; p->n = N_tilde * model->nv; p->m0 = N_tilde * d.nc;
    {   /* cut budgets: a negative value asks for the size-scaled default (300 rows / 80 Gomory + 10 rounding cuts per round up to the cfg3
         * shape).  Round 1 ran 200 / 40 / 20 over 8 rounds and withdrew anything deeper after one false optimality claim; that claim was
         * the dual simplex's tiny-pivot breakdown (DESIGN section 4), and with the guard the deeper loop is clean against HiGHS
         * (tests/test_gpu_loop.py) and 5 % faster: Gomory cuts are derived eight at a time and nearly free, rounding cuts are not. */
        const int nbin = N_tilde * (d.nu_l + d.ndelta + d.nmu_l);
        /* round 3: 20 rounding cuts per round (was 10: 2048 bench instances on the CPU restatement: 12 % fewer row updates, 9 -> 3 node-limited;
         * steady-state closed-loop instances: 18 % fewer), and above the cfg4 size the loop deepens with the number of binaries -- cfg5 (784
         * binaries, NodeLimit 400, 256 instances): 10 rounds / 441 rows / 78 rounding cuts 47 % proven, 19 rounds / 882 rows / 156 rounding cuts 59 % */
        if (p->opts.max_cuts < 0) p->opts.max_cuts = nbin <= 400 ? std::max(300, p->m0 / 4) : p->m0 / 2;
        if (p->opts.cuts_per_round < 0) p->opts.cuts_per_round = std::max(80, nbin / 5);
        if (p->opts.mir_per_round < 0) p->opts.mir_per_round = nbin <= 400 ? 20 : nbin / 5;
        if (p->opts.cut_rounds < 0) p->opts.cut_rounds = std::max(10, std::min(30, nbin / 40));
    }
    if (p->opts.cut_rounds <= 0 || p->opts.max_cuts == 0) { p->opts.cut_rounds = 0; }
    p->nx = d.nx; p->nW = N_tilde * d.nomega; p->n_models = model->n_models;
    const int n = p->n, m0 = p->m0, M = p->n_models;
    int rc = MLD_OK;
    // 1. tightened copy of the model, condensed on device (K1+K2)
    {
        std::vector<std::vector<double>> hm = model->h_mats;
        const int steps = model->tv_N > 0 ? model->tv_N : 1;      /* time-varying horizon: every step model is tightened on its own rows */
        if (p->opts.presolve & 2) for (int k = 0; k < M * steps; ++k) tighten::run(d, hm, (size_t)k);
        const double *ptrs[20];
        for (int k = 0; k < 20; ++k) ptrs[k] = hm[k].empty() ? nullptr : hm[k].data();
        mld_model *t = nullptr;
        if ((rc = model_create_impl(&t, &d, M, model->tv_N, ptrs))) return rc;
        p->tight.reset(t);
        if ((rc = condense_model_device(t, N_tilde, nullptr, 0))) return rc;
    }
    // 2. variable layout: bounds + binaries  (variables.py:189-243 ; mld_model.py:294-345)
    std::vector<double> lb((size_t)n, -std::numeric_limits<double>::infinity()), ub((size_t)n, std::numeric_limits<double>::infinity());
    std::vector<unsigned char> is_int(n, 0);
    std::vector<int> bins;
    for (int k = 0; k < N_tilde; ++k) {
        const int o = k * p->nv;
        for (int j = d.nu - d.nu_l; j < d.nu; ++j) is_int[o + j] = 1;
        for (int j = 0; j < d.ndelta; ++j) is_int[o + d.nu + j] = 1;
        const int omu = d.nu + d.ndelta + d.nz;
        for (int j = 0; j < d.nmu; ++j) lb[o + omu + j] = 0.0;
        for (int j = d.nmu - d.nmu_l; j < d.nmu; ++j) is_int[o + omu + j] = 1;
    }
    for (int j = 0; j < n; ++j) if (is_int[j]) { lb[j] = 0.0; ub[j] = 1.0; bins.push_back(j); }
    p->nb = (int)bins.size();
    // 3. scaling from the tightened H_v (host, once per problem) and the scaled dense G
    std::vector<double> G((size_t)m0 * n * M), rs((size_t)m0 * M, 1.0), cs((size_t)n * M, 1.0);
    if (m0 && n) {
        hipError_t e = hipMemcpy(G.data(), p->tight->d_out[O_HV], sizeof(double) * G.size(), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { mld_set_error("D2H H_v: %s", hipGetErrorString(e)); return MLD_ERR_HIP; }
    }
    for (int k = 0; k < M; ++k) {
        double *g = G.data() + (size_t)k * m0 * n, *r = rs.data() + (size_t)k * m0, *c = cs.data() + (size_t)k * n;
        std::vector<double> cmax(n);
        for (int pass = 0; pass < 3; ++pass) {
            for (int i = 0; i < m0; ++i) {
                double mx = 0;
                for (int j = 0; j < n; ++j) mx = std::max(mx, std::fabs(g[(size_t)i * n + j]) * r[i] * c[j]);
                if (mx > 0) r[i] /= mx;
            }
            std::fill(cmax.begin(), cmax.end(), 0.0);
            for (int i = 0; i < m0; ++i)
                for (int j = 0; j < n; ++j) cmax[j] = std::max(cmax[j], std::fabs(g[(size_t)i * n + j]) * r[i] * c[j]);
            for (int j = 0; j < n; ++j) if (!is_int[j] && cmax[j] > 0) c[j] /= cmax[j];
        }
        for (int i = 0; i < m0; ++i) r[i] = std::exp2(std::rint(std::log2(r[i])));
        for (int j = 0; j < n; ++j) c[j] = std::exp2(std::rint(std::log2(c[j])));
        for (int i = 0; i < m0; ++i)
            for (int j = 0; j < n; ++j) g[(size_t)i * n + j] *= r[i] * c[j];
    }
    std::vector<double> lbs((size_t)n * M), ubs((size_t)n * M);
    for (int k = 0; k < M; ++k)
        for (int j = 0; j < n; ++j) { lbs[(size_t)k * n + j] = lb[j] / cs[(size_t)k * n + j]; ubs[(size_t)k * n + j] = ub[j] / cs[(size_t)k * n + j]; }
    if ((rc = upload(p->d_Gs, G)) || (rc = upload(p->d_rs, rs)) || (rc = upload(p->d_cs, cs)) || (rc = upload(p->d_lb, lbs)) ||
        (rc = upload(p->d_ub, ubs))) return rc;
    {
        int cap = 0;
        for (size_t r = 0; r < (size_t)M * m0; ++r) {
            int cnt = 0;
            for (int j = 0; j < n; ++j) cnt += (is_int[j] && G[r * n + j] != 0.0);
            cap = std::max(cap, cnt);
        }
        p->mir_cap = (cap + 7) / 8 * 8;
    }
    if (m0 && n) {   /* largest activity of every scaled row under the model's own bounds (k_solve's s_mark_dead compares it with the instance's right-hand side) */
        std::vector<double> am((size_t)m0 * M);
        for (int k = 0; k < M; ++k)
            for (int i = 0; i < m0; ++i) {
                const double *g = G.data() + ((size_t)k * m0 + i) * n;
                double act = 0.0; bool inf = false;
                for (int j = 0; j < n; ++j) {
                    const double gj = g[j];
                    if (gj > 0.0) { const double hi = ubs[(size_t)k * n + j]; if (hi < 0.5 * S_BIG) act += gj * hi; else inf = true; }
                    else if (gj < 0.0) { const double lo = lbs[(size_t)k * n + j]; if (lo > -0.5 * S_BIG) act += gj * lo; else inf = true; }
                }
                am[(size_t)k * m0 + i] = inf ? (double)INFINITY : act;
            }
        if ((rc = upload(p->d_actmax, am))) return rc;
    }
    if (m0 && n && (p->opts.presolve & 4) && m0 < 65536 && n < 65536) {
        /* the scaled rows once more, sparse (by row and by column): the per-instance presolve walks the non-zeros only (cfg4: 5 450 of 287 500) */
        size_t cap = 1;
        for (int k = 0; k < M; ++k) { size_t c = 0; const double *g = G.data() + (size_t)k * m0 * n; for (size_t e = 0; e < (size_t)m0 * n; ++e) c += g[e] != 0.0; cap = std::max(cap, c); }
        cap = (cap + 7) / 8 * 8;
        std::vector<int> rptr((size_t)M * (m0 + 1)), cptr((size_t)M * (n + 1));
        std::vector<unsigned short> rcol((size_t)M * cap, 0), crow((size_t)M * cap, 0);
        std::vector<double> rval((size_t)M * cap, 0.0), cval((size_t)M * cap, 0.0);
        for (int k = 0; k < M; ++k) {
            const double *g = G.data() + (size_t)k * m0 * n;
            int *rp = rptr.data() + (size_t)k * (m0 + 1), *cp = cptr.data() + (size_t)k * (n + 1);
            size_t e = 0;
            for (int i = 0; i < m0; ++i) {
                rp[i] = (int)e;
                for (int j = 0; j < n; ++j) if (g[(size_t)i * n + j] != 0.0) { rcol[(size_t)k * cap + e] = (unsigned short)j; rval[(size_t)k * cap + e] = g[(size_t)i * n + j]; ++e; }
            }
            rp[m0] = (int)e;
            e = 0;
            for (int j = 0; j < n; ++j) {
                cp[j] = (int)e;
                for (int i = 0; i < m0; ++i) if (g[(size_t)i * n + j] != 0.0) { crow[(size_t)k * cap + e] = (unsigned short)i; cval[(size_t)k * cap + e] = g[(size_t)i * n + j]; ++e; }
            }
            cp[n] = (int)e;
        }
        p->nnz_cap = (int)cap;
        if ((rc = upload(p->d_csr_ptr, rptr)) || (rc = upload(p->d_csc_ptr, cptr)) || (rc = upload(p->d_csr_col, rcol)) || (rc = upload(p->d_csc_row, crow)) ||
            (rc = upload(p->d_csr_val, rval)) || (rc = upload(p->d_csc_val, cval))) return rc;
    }
    {
        std::vector<int> pos(n, -1), perm(n);
        for (int k = 0; k < p->nb; ++k) pos[bins[k]] = k;
        // dictionary column order: position-major (all horizon steps of one per-step variable adjacent), so that the
        // non-zeros of a pivot row -- which follow the per-step coupling pattern -- fall into few 64-byte sectors
        int c = 0;
        for (int q = 0; q < p->nv; ++q) for (int k = 0; k < N_tilde; ++k) perm[c++] = k * p->nv + q;
        std::vector<double> Gp((size_t)M * m0 * n);
        for (size_t r = 0; r < (size_t)M * m0; ++r)
            for (int k = 0; k < n; ++k) Gp[r * n + k] = G[r * n + perm[k]];
        if ((rc = upload(p->d_is_int, is_int)) || (rc = upload(p->d_bins, bins)) || (rc = upload(p->d_binpos, pos)) || (rc = upload(p->d_colperm, perm)) ||
            (rc = upload(p->d_Gp, Gp))) return rc;
        hipError_t e = p->d_qs.alloc((size_t)std::max(1, n) * M);
        if (e == hipSuccess) e = p->d_q0.alloc((size_t)std::max(1, n) * M);
        if (e == hipSuccess) e = p->d_cx.alloc((size_t)std::max(1, p->nx) * M);
        if (e == hipSuccess) e = p->d_cw.alloc((size_t)std::max(1, p->nW) * M);
        if (e == hipSuccess) e = p->d_c0.alloc(M);
        if (e == hipSuccess) e = p->d_counter.alloc(1);
        if (e != hipSuccess) { mld_set_error("problem alloc: %s", hipGetErrorString(e)); return MLD_ERR_HIP; }
    }
    // 3b. LDS-resident LP path: Toeplitz-compatible equilibration (one factor per row-in-step and per variable-in-step, so that the
    //     scaled H_v is still block Toeplitz) of the tightened model's lag blocks; only time-invariant models
    if (model->tv_N == 0 && m0 && n && p->tight->d_blocks) {
        const int N = N_tilde, nc = d.nc, nv = p->nv;
        const CondLayout &L = p->tight->lay;
        std::vector<double> blk((size_t)M * N * nc * nv), rst((size_t)M * m0), cst((size_t)M * n), lbt((size_t)M * n), ubt((size_t)M * n);
        bool okc = true;
        for (int k = 0; k < M && okc; ++k)
            okc = hipMemcpy(blk.data() + (size_t)k * N * nc * nv, p->tight->d_blocks + (size_t)k * L.blk_stride + L.offV[2], sizeof(double) * N * nc * nv, hipMemcpyDeviceToHost) == hipSuccess;
        if (okc) {
            for (int k = 0; k < M; ++k) {
                double *b = blk.data() + (size_t)k * N * nc * nv;
                std::vector<double> r(nc, 1.0), c(nv, 1.0), cmax(nv);
                for (int pass = 0; pass < 3; ++pass) {
                    for (int i = 0; i < nc; ++i) {
                        double mx = 0;
                        for (int lag = 0; lag < N; ++lag) for (int j = 0; j < nv; ++j) mx = std::max(mx, std::fabs(b[((size_t)lag * nc + i) * nv + j]) * r[i] * c[j]);
                        if (mx > 0) r[i] /= mx;
                    }
                    std::fill(cmax.begin(), cmax.end(), 0.0);
                    for (int lag = 0; lag < N; ++lag) for (int i = 0; i < nc; ++i) for (int j = 0; j < nv; ++j) cmax[j] = std::max(cmax[j], std::fabs(b[((size_t)lag * nc + i) * nv + j]) * r[i] * c[j]);
                    for (int j = 0; j < nv; ++j) if (!is_int[j] && cmax[j] > 0) c[j] /= cmax[j];
                }
                for (int i = 0; i < nc; ++i) r[i] = std::exp2(std::rint(std::log2(r[i])));
                for (int j = 0; j < nv; ++j) c[j] = std::exp2(std::rint(std::log2(c[j])));
                for (int lag = 0; lag < N; ++lag) for (int i = 0; i < nc; ++i) for (int j = 0; j < nv; ++j) b[((size_t)lag * nc + i) * nv + j] *= r[i] * c[j];
                for (int i = 0; i < m0; ++i) rst[(size_t)k * m0 + i] = r[i % nc];
                for (int j = 0; j < n; ++j) { const double cj = c[j % nv]; cst[(size_t)k * n + j] = cj; lbt[(size_t)k * n + j] = lb[j] / cj; ubt[(size_t)k * n + j] = ub[j] / cj; }
            }
            LpShape &LS = p->LS;
            LS.n = n; LS.m = m0; LS.N = N; LS.nc = nc; LS.nv = nv; LS.nx = p->nx; LS.nW = p->nW; LS.max_pivots = p->opts.max_pivots;
            int dev = 0; hipDeviceProp_t prop;
            (void)hipGetDevice(&dev); (void)hipGetDeviceProperties(&prop, dev);
            const size_t budget = 160 * 1024 - 1024;      /* CDNA4: 160 KB per workgroup; static LDS of the kernel is < 1 KB */
            auto dbl_for = [&](int kc) { return (size_t)N * nc * nv + (size_t)kc * (kc + 1) + 3 * (size_t)n + m0 + 6 * (size_t)kc + (2 * ((size_t)n + m0 + 4 * (size_t)kc) + 3 * (size_t)n + m0 + 7) / 8 + 1; };   /* doubles before the fp32 bounds */
            auto lds_for = [&](int kc) { return sizeof(double) * dbl_for(kc) + sizeof(float) * 2 * (size_t)n + 64; };
            int kc = std::min(128, std::min(n, m0));
            if (p->opts.reserved & MLD_DBG_LP_LDS_K24) kc = std::min(kc, 24);      /* diagnostics: a small working-basis capacity so that the overflow fall-back runs */
            while (kc >= 8 && lds_for(kc) > budget) kc -= 4;
            if (kc >= 8 && n < 32767 && m0 < 32767) {
                LS.kcap = kc; LS.ldw = kc + 1; LS.f32_off = (int)dbl_for(kc); p->lp_lds_bytes = lds_for(kc);
                p->lp_slots = prop.multiProcessorCount;
                if ((rc = upload(p->d_blk_t, blk)) || (rc = upload(p->d_rs_t, rst)) || (rc = upload(p->d_cs_t, cst)) || (rc = upload(p->d_lb_t, lbt)) || (rc = upload(p->d_ub_t, ubt))) return rc;
                const hipError_t e = p->d_qs_t.alloc((size_t)n * M);
                if (e != hipSuccess) { mld_set_error("lp path alloc: %s", hipGetErrorString(e)); return MLD_ERR_HIP; }
                p->lp_ok = true;
            }
        }
    }
    // 3c. small-problem path (MLD_SMALL_LDS): eligible when the dictionary with its per-basis state and the search stack fits a wave's share of LDS
    if ((p->opts.flags & MLD_SMALL_LDS) && m0 && n && sizeof(double) * sm_wave_doubles(n, m0, p->nb) <= SM_WAVE_BUDGET) {
        SmShape &SS = p->SS;
        SS.n = n; SS.m = m0; SS.ld = n | 1; SS.nb = p->nb; SS.nx = p->nx; SS.nW = p->nW;
        SS.cp = 1; SS.cshift = 0;
        while (SS.cp < 64 && SS.cp < n) { SS.cp <<= 1; SS.cshift++; }
        SS.wave_doubles = (int)sm_wave_doubles(n, m0, p->nb);
        p->small_lds_bytes = sizeof(double) * (size_t)SS.wave_doubles * SM_WAVES;
        int dev = 0, per_cu = 0; hipDeviceProp_t prop;
        (void)hipGetDevice(&dev); (void)hipGetDeviceProperties(&prop, dev);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_small_milp, SM_NT, p->small_lds_bytes) != hipSuccess || per_cu < 1) per_cu = 1;
        p->small_slots = per_cu * prop.multiProcessorCount;
        HIP_TRY(p->d_declined.alloc(1));
        p->small_ok = true;
    }
    // 4. cost (K4)
    if ((rc = set_cost_impl(p.get(), cost))) return rc;
    // 5. workspace: one dictionary per resident workgroup
    if ((rc = build_shape(p.get()))) return rc;
    {
        int dev = 0; hipDeviceProp_t prop;
        (void)hipGetDevice(&dev); (void)hipGetDeviceProperties(&prop, dev);
        if (p->lds_bytes > 48 * 1024 && p->lds_bytes <= 150 * 1024)
            (void)hipFuncSetAttribute((const void *)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds_bytes);
        int per_cu = 0;   /* resident workgroups per CU for this LDS size (the kernel's 256 VGPRs allow one): a larger grid would only queue */
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_solve, SOL_NT, p->lds_bytes) != hipSuccess || per_cu < 1) per_cu = 1;
        p->n_slots = p->opts.n_slots > 0 ? p->opts.n_slots : per_cu * prop.multiProcessorCount;
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        while (p->n_slots > 1 && (size_t)p->n_slots * p->S.ws_stride > free_b / 2) p->n_slots /= 2;
        if (p->lds_bytes > 150 * 1024) { mld_set_error("problem too large for LDS staging (%zu bytes)", p->lds_bytes); return MLD_ERR_UNSUPPORTED; }
        hipError_t e = p->d_ws.alloc((size_t)p->n_slots * p->S.ws_stride);
        if (e != hipSuccess) { mld_set_error("workspace alloc (%zu MB): %s", (size_t)p->n_slots * p->S.ws_stride >> 20, hipGetErrorString(e)); return MLD_ERR_HIP; }
        if (p->lds_bytes > 48 * 1024)
            (void)hipFuncSetAttribute((const void *)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds_bytes);
    }
    *out = p.release();
    return MLD_OK;
}

int mld_problem_set_cost(mld_problem_t *p, const mld_cost *cost)
{
    if (int rc = entry_guard(p, "mld_problem_set_cost", false, nullptr)) return rc;
    if (!p) { mld_set_error("null problem"); return MLD_ERR_INVALID; }
    return set_cost_impl(p, cost);
}

int mld_cost_assemble(mld_problem_t *p, double *P, double *q0, double *Qx, double *Qw)
{
    if (!p) { mld_set_error("null problem"); return MLD_ERR_INVALID; }
    const size_t n = p->n, M = p->n_models;
    if (q0) HIP_TRY(hipMemcpy(q0, p->d_q0, sizeof(double) * n * M, hipMemcpyDeviceToHost));
    if (P) { if (p->d_P) HIP_TRY(hipMemcpy(P, p->d_P, sizeof(double) * n * n * M, hipMemcpyDeviceToHost)); else memset(P, 0, sizeof(double) * n * n * M); }
    if (Qx && p->nx) { if (p->d_Qx) HIP_TRY(hipMemcpy(Qx, p->d_Qx, sizeof(double) * n * p->nx * M, hipMemcpyDeviceToHost)); else memset(Qx, 0, sizeof(double) * n * p->nx * M); }
    if (Qw && p->nW) { if (p->d_Qw) HIP_TRY(hipMemcpy(Qw, p->d_Qw, sizeof(double) * n * p->nW * M, hipMemcpyDeviceToHost)); else memset(Qw, 0, sizeof(double) * n * p->nW * M); }
    return MLD_OK;
}

int mld_problem_get_opts(mld_problem_t *p, mld_opts *out)
{
    if (!p || !out) { mld_set_error("mld_problem_get_opts: bad arguments"); return MLD_ERR_INVALID; }
    *out = p->opts;      /* with every size-scaled default resolved */
    out->n_slots = p->n_slots;
    return MLD_OK;
}

int mld_problem_set_opts(mld_problem_t *p, const mld_opts *o)
{
    if (int rc = entry_guard(p, "mld_problem_set_opts", false, nullptr)) return rc;
    if (!p || !o) { mld_set_error("mld_problem_set_opts: bad arguments"); return MLD_ERR_INVALID; }
    /* limits and tolerances only: the workspace layout (max_cuts, n_slots) and the tightened model (presolve) stay.  Every check comes BEFORE the first
     * assignment: a refused call changes nothing (ADVICE r3). */
    if (o->flags != p->opts.flags) { mld_set_error("mld_problem_set_opts: flags (MLD_F32, MLD_SMALL_LDS) are fixed at mld_problem_create -- they decide how the cost is assembled and which solve paths exist"); return MLD_ERR_INVALID; }
    if (!(o->gap_abs >= 0.0) || !(o->gap_rel >= 0.0) || o->max_nodes < 1 || o->max_pivots < 1) { mld_set_error("mld_problem_set_opts: gaps must be >= 0, node / pivot limits >= 1"); return MLD_ERR_INVALID; }
    p->opts.gap_abs = o->gap_abs; p->opts.gap_rel = o->gap_rel; p->opts.max_nodes = o->max_nodes; p->opts.max_pivots = o->max_pivots;
    p->opts.reserved = o->reserved;
    if (o->time_limit >= 0.0) p->opts.time_limit = o->time_limit;      /* (negative keeps the current value) */
    if (o->cut_rounds >= 0) p->opts.cut_rounds = p->opts.max_cuts > 0 ? o->cut_rounds : 0;
    if (o->cuts_per_round >= 0) p->opts.cuts_per_round = o->cuts_per_round;
    if (o->mir_per_round >= 0) p->opts.mir_per_round = o->mir_per_round;
    SolverShape &S = p->S;
    S.cuts_per_round = p->opts.cuts_per_round; S.cut_rounds = p->opts.cut_rounds; S.mir_per_round = p->opts.mir_per_round;
    S.max_nodes = p->opts.max_nodes; S.max_pivots = p->opts.max_pivots; S.gap_abs = p->opts.gap_abs; S.gap_rel = p->opts.gap_rel;
    S.debug = p->opts.reserved; S.time_ticks = time_limit_ticks(p->opts.time_limit);
    return MLD_OK;
}

} // extern "C"
