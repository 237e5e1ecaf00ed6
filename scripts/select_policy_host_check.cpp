// What mld_rollout_select_policy adds to the rollout and selection kernels (pyhybridcontrol_amd/csrc/rollout.inc, plan_select.inc), on the CPU under the host
// sanitizers: with SM_HOST a "wave" is one lane and the LDS block plain memory.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/select_policy_host_check.cpp -o /tmp/select_policy_host_check && /tmp/select_policy_host_check
//
// 1. ro_run<true> with a table whose every channel is passed through against ro_run<false> on the same inputs, bit for bit -- what makes a plan or sequence
//    candidate of the candidate-policy kernels the candidate it is in k_rollout_cand -- and switches == 0.  The one-tank model of scripts/policy_host_check.cpp.
// 2. The table index arithmetic (ro_cand_table, ro_cand_rows, ro_cand_input) at cp = n_seq - 1, n_seq, P - 1 and everywhere between, over a table buffer of
//    exactly (P - n_seq + 1) n_models nu (nx + 5) doubles, so that the sanitizer sees a read past it; every row carries a mark that names it.
// 3. The input rule of k_select_inputs (sel_source, sel_policy_row0, ro_cand_input) over its index edges -- no choice, the plan, the first and last sequence,
//    the first and last policy -- as a serial restatement of the kernel's loop against a naive one, every buffer exactly as long as the kernel may touch.
#define SM_HOST
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mldgpu.h"
#include "rollout.inc"
#include "plan_select.inc"

static int failures = 0;
static bool same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
static void fail(const char *what, long long i, double got, double want)
{
    printf("FAIL %s[%lld]: got %.17g, expected %.17g\n", what, i, got, want);
    ++failures;
}

// ---- 1. the all-pass-through table against the open-loop instantiation
static void pass_through_is_open_loop()
{
    const double BM = 10.0;
    const int nx = 1, nu = 1, nw = 1, nv = 4, nmu = 1, ny = 1, n = 3, m = 7, nc = 7;
    const double E[7] = {0, 0, 0, 0, 0, 0, 1}, F1[7] = {1, -1, 0, 0, -1, 1, 0}, F2[7] = {-BM, BM, -BM, 0, BM, BM, 0}, F3[7] = {0, 0, 1, -1, 1, -1, 0};
    const double F4[7] = {-1, 1, 0, 0, 1, -1, 0}, Psi[7] = {0, 0, 0, 0, 0, 0, -1}, f5[7] = {0, BM, 0, 0, BM, BM, 4}, Gy[7] = {0, 0, 0, 0, 0, 0, 0};
    const double A[1] = {0.5}, B4[1] = {0}, b5[1] = {0.5}, C[1] = {1}, D4[1] = {0}, d5[1] = {0};
    const double Bv[4] = {0, 0, 1, 0}, Dv[4] = {0, 0, 1, 0};
    std::vector<double> Fv((size_t)nc * nv), G((size_t)m * n), Hx(m), Hw((size_t)m * 2), H5(m), rs(m, 1.0);
    for (int i = 0; i < m; ++i) {
        Fv[i * nv + 0] = F1[i]; Fv[i * nv + 1] = F2[i]; Fv[i * nv + 2] = F3[i]; Fv[i * nv + 3] = Psi[i];
        G[i * n + 0] = F2[i]; G[i * n + 1] = F3[i]; G[i * n + 2] = Psi[i];
        Hx[i] = -E[i]; Hw[i * 2 + 0] = -F4[i]; Hw[i * 2 + 1] = -F1[i]; H5[i] = f5[i];
    }
    const double q[3] = {0, 0, 1}, lb[3] = {0, -BM, 0}, ub[3] = {1, BM, S_INF}, cs[3] = {1, 1, 1};
    const unsigned char is_int[3] = {1, 0, 0}; const int bins[1] = {0};
    const int K = 6;
    const double seqs[3][6] = {{3, 1, 4, 1, 0.3, 2.7}, {0, 0, 0, 0, 0, 0}, {4, 4, 4, 4, 4, 4}};
    const double oms[3][6] = {{1, 2, 0.5, 0, 1.1, 0.7}, {1, 1, 1, 1, 1, 1}, {0.1, 0.2, 0.3, 0.4, 0.5, 0.6}};
    const double cw[24] = {1, 0.5, 2, 3, 1.5, 0.25, 1, 1, 2, 2, 2, 2, 0.1, 0.2, 0.3, 0.4, 1, 0.5, 2, 3, 1.5, 0.25, 1, 1};
    for (int s = 0; s < 3; ++s)
        for (int c = 0; c < 3; ++c) {
            SmShape S{};
            S.n = n; S.m = m; S.ld = n | 1; S.nb = 1; S.nx = nx; S.nW = nw + nu; S.cp = 1; S.cshift = 0;
            S.max_nodes = 100; S.max_pivots = 1000; S.gap_abs = 1e-9; S.gap_rel = 0.0;
            S.wave_doubles = (int)sm_wave_doubles(n, m, 1);
            RoModel M{};
            M.nx = nx; M.nu = nu; M.nw = nw; M.nv = nv; M.nmu = nmu; M.ny = ny; M.nc = nc; M.m = m; M.n = n;
            M.P = PlantMats{A, B4, b5, C, D4, d5, E, F4, f5, Gy, Bv, Dv, Fv.data()};
            M.Hx = Hx.data(); M.Hw = Hw.data(); M.H5 = H5.data(); M.rs = rs.data();
            std::vector<double> tab((size_t)nu * (nx + POL_TAIL), 0.0);      // the host's last table: all zero, mode 0
            M.pol = tab.data();
            SmArgs Aa{};
            Aa.G = G.data(); Aa.q = q; Aa.lb = lb; Aa.ub = ub; Aa.cs = cs; Aa.is_int = is_int; Aa.bins = bins;
            const double x0 = 2.0 + 0.75 * c, up[1] = {7.0};
            std::vector<double> u(seqs[s], seqs[s] + K), om(oms[c], oms[c] + K), w(cw, cw + K * nv);
            RoResult R[2];
            std::vector<double> x[2], v[2], y[2], vio[2];
            std::vector<int> row[2];
            for (int pass = 0; pass < 2; ++pass) {
                std::vector<double> mem((size_t)S.wave_doubles), stg(ro_stage_doubles(nx, nu, nw, m, nv, ny));
                x[pass].assign((size_t)(K + 1) * nx, -7.0); v[pass].assign((size_t)K * nv, -7.0); y[pass].assign((size_t)K * ny, -7.0); vio[pass].assign(K, -7.0);
                row[pass].assign(K, -7);
                RoTraj T{};
                T.K = K; T.x0 = &x0; T.u = u.data(); T.u_step = nu; T.om = om.data(); T.cw = w.data();
                T.x = x[pass].data(); T.v = v[pass].data(); T.y = y[pass].data(); T.vio = vio[pass].data(); T.row = row[pass].data(); T.u_prev = up;
                R[pass] = RoResult{};
                R[pass].switches = -7;
                if (pass == 0) ro_run<false>(S, M, mem.data(), stg.data(), Aa, T, 0, R[0]);
                else ro_run<true>(S, M, mem.data(), stg.data(), Aa, T, 0, R[1]);
            }
            const long long id = 3 * s + c;
            if (R[0].end_status != RO_COMPLETE || R[1].end_status != RO_COMPLETE) fail("end_status", id, R[1].end_status, RO_COMPLETE);
            if (R[0].switches != -7 || R[1].switches != 0) fail("switches (open loop untouched, pass-through 0)", id, R[1].switches, 0);
            if (!same(R[0].cost, R[1].cost)) fail("cost", id, R[1].cost, R[0].cost);
            if (!same(R[0].mu_total, R[1].mu_total)) fail("mu_total", id, R[1].mu_total, R[0].mu_total);
            if (!same(R[0].worst_vio, R[1].worst_vio)) fail("worst_vio", id, R[1].worst_vio, R[0].worst_vio);
            if (R[0].worst_step != R[1].worst_step || R[0].worst_row != R[1].worst_row || R[0].steps_done != R[1].steps_done) fail("worst_step / worst_row / steps_done", id, R[1].worst_step, R[0].worst_step);
            if (memcmp(x[0].data(), x[1].data(), sizeof(double) * x[0].size())) fail("x", id, 0, 0);
            if (memcmp(v[0].data(), v[1].data(), sizeof(double) * v[0].size())) fail("v", id, 0, 0);
            if (memcmp(y[0].data(), y[1].data(), sizeof(double) * y[0].size())) fail("y", id, 0, 0);
            if (memcmp(vio[0].data(), vio[1].data(), sizeof(double) * vio[0].size())) fail("cons_vio", id, 0, 0);
            if (memcmp(row[0].data(), row[1].data(), sizeof(int) * row[0].size())) fail("cons_row", id, 0, 0);
            for (int k = 0; k < K; ++k) if (!same(v[1][(size_t)k * nv], u[k])) fail("u_k of the pass-through table", k, v[1][(size_t)k * nv], u[k]);
        }
}

// the tables of a call: (T + 1, n_models, nu, nx + 5), row (t, m, j) marked -- u_on = mark(t, m, j), on_at = +huge so that the rule returns the mark --, the
// last table all zero
static double mark(int t, int m, int j) { return 1000.0 * (t + 1) + 10.0 * m + j + 0.5; }
static std::vector<double> marked_tables(int T, int n_models, int nu, int nx)
{
    const size_t row = (size_t)nx + POL_TAIL;
    std::vector<double> tabs((size_t)(T + 1) * n_models * nu * row, 0.0);
    for (int t = 0; t < T; ++t)
        for (int m = 0; m < n_models; ++m)
            for (int j = 0; j < nu; ++j) {
                double *r = tabs.data() + (((size_t)t * n_models + m) * nu + j) * row;
                for (int i = 0; i < nx; ++i) r[i] = i == j % nx ? 1.0 : 0.0;
                r[nx + POL_ON_AT] = 1e300; r[nx + POL_OFF_AT] = 1e300; r[nx + POL_U_ON] = mark(t, m, j); r[nx + POL_U_OFF] = -1.0; r[nx + POL_MODE] = 1.0;
            }
    return tabs;
}

// ---- 2. the table of a candidate
static void table_index()
{
    const int n_models = 3, nu = 2, nx = 3;
    const size_t tab_len = (size_t)nu * (nx + POL_TAIL);
    const double x0[3] = {1, 2, 3};
    int checked = 0;
    for (int T = 1; T <= 5; ++T)
        for (int n_seq = 0; n_seq <= 4; ++n_seq) {
            const int P = n_seq + T;
            const std::vector<double> tabs = marked_tables(T, n_models, nu, nx);
            for (int cp = 0; cp < P; ++cp) {
                const size_t want = cp >= n_seq ? (size_t)(cp - n_seq) : (size_t)T;
                if (ro_cand_table(cp, n_seq, P) != want) fail("ro_cand_table", cp, (double)ro_cand_table(cp, n_seq, P), (double)want);
                for (int m = 0; m < n_models; ++m) {
                    const double *rows = ro_cand_rows(tabs.data(), tab_len, n_models, cp, n_seq, P, m);
                    if (rows != tabs.data() + (want * n_models + m) * tab_len) fail("ro_cand_rows", cp, (double)(rows - tabs.data()), (double)((want * n_models + m) * tab_len));
                    for (int j = 0; j < nu; ++j) {
                        const double mode = rows[(size_t)j * (nx + POL_TAIL) + nx + POL_MODE];
                        if (cp < n_seq) { if (mode != 0.0) fail("a sequence candidate's table passes every channel through", cp, mode, 0.0); }
                        else {
                            const double got = ro_cand_input(tabs.data(), tab_len, n_models, cp, n_seq, P, m, j, nx, x0, 0.0);
                            if (!same(got, mark(cp - n_seq, m, j))) fail("ro_cand_input", cp, got, mark(cp - n_seq, m, j));
                        }
                        ++checked;
                    }
                }
            }
            /* the three edges by name */
            if (n_seq > 0 && ro_cand_table(n_seq - 1, n_seq, P) != (size_t)T) fail("cp = n_seq - 1", n_seq, 0, 0);
            if (ro_cand_table(n_seq, n_seq, P) != 0) fail("cp = n_seq", n_seq, 0, 0);
            if (ro_cand_table(P - 1, n_seq, P) != (size_t)(T - 1)) fail("cp = P - 1", P, 0, 0);
        }
    printf("table index: %d (candidate, model, channel) rows, each the one its mark names\n", checked);
}

// ---- 3. k_select_inputs' loop, serially: lanes 0 .. 63 of the wave of instance b
static void select_inputs()
{
    const double qnan = __builtin_nan("");
    int checked = 0;
    for (int plan_first = 0; plan_first <= 1; ++plan_first)
        for (int n_own = 0; n_own <= 2; ++n_own)
            for (int T = 1; T <= 2; ++T)
                for (int K = 1; K <= 3; K += 2)
                    for (int with_u = 0; with_u <= 1; ++with_u) {
                        const int n_models = 2, nu = 3, nx = 3, n_seq = plan_first + n_own, P = n_seq + T, batch = P + 2, nv = 5, n = 40;
                        const size_t tab_len = (size_t)nu * (nx + POL_TAIL), Knu = (size_t)K * nu;
                        const std::vector<double> tabs = marked_tables(T, n_models, nu, nx);
                        std::vector<double> u_cand((size_t)batch * n_own * Knu), plan((size_t)batch * n), x0((size_t)batch * nx, 1.0), u_prev((size_t)batch * nu, 0.0);
                        for (size_t i = 0; i < u_cand.size(); ++i) u_cand[i] = 0.25 * (double)i + 1.0;
                        for (size_t i = 0; i < plan.size(); ++i) plan[i] = -0.5 * (double)i - 1.0;
                        std::vector<int> choice(batch), midx(batch);
                        for (int b = 0; b < batch; ++b) { choice[b] = b - 1 < P ? b - 1 : P - 1; midx[b] = b % n_models; }      /* -1, 0, .., P - 1, P - 1 */
                        std::vector<double> u(with_u ? (size_t)batch * Knu : 0, -7.0), u0((size_t)batch * nu, -7.0);
                        for (int b = 0; b < batch; ++b)
                            for (int lane = 0; lane < 64; ++lane) {
                                int row;
                                const int from = sel_source(choice[b], plan_first, n_seq, row);
                                if (from == SEL_FROM_POLICY) {
                                    for (size_t e = lane; e < (with_u ? Knu : (size_t)nu); e += 64) {
                                        double t = qnan;
                                        if (sel_policy_row0(e, nu))
                                            t = ro_cand_input(tabs.data(), tab_len, n_models, choice[b], n_seq, P, midx[b], (int)e, nx, x0.data() + (size_t)b * nx, u_prev[(size_t)b * nu + e]);
                                        if (e < (size_t)nu) u0[(size_t)b * nu + e] = t;
                                        if (with_u) u[(size_t)b * Knu + e] = t;
                                    }
                                    continue;
                                }
                                const double *src = nullptr; size_t step = nu;
                                if (from == SEL_FROM_PLAN) { src = plan.data() + (size_t)b * n; step = nv; }
                                else if (from == SEL_FROM_SEQ) src = u_cand.data() + ((size_t)b * (n_seq - plan_first) + row) * Knu;
                                if (with_u) for (size_t e = lane; e < Knu; e += 64) { const size_t k = e / nu, j = e - k * nu; u[(size_t)b * Knu + e] = src ? src[k * step + j] : qnan; }
                                for (size_t j = lane; j < (size_t)nu; j += 64) u0[(size_t)b * nu + j] = src ? src[j] : qnan;
                            }
                        /* the naive restatement */
                        for (int b = 0; b < batch; ++b)
                            for (int k = 0; k < K; ++k)
                                for (int j = 0; j < nu; ++j) {
                                    const int pick = choice[b];
                                    double want;
                                    if (pick < 0) want = qnan;
                                    else if (pick >= n_seq) want = k == 0 ? mark(pick - n_seq, midx[b], j) : qnan;
                                    else if (plan_first && pick == 0) want = plan[(size_t)b * n + (size_t)k * nv + j];
                                    else want = u_cand[(((size_t)b * n_own + (pick - plan_first)) * K + k) * nu + j];
                                    if (with_u) { const double got = u[((size_t)b * K + k) * nu + j]; if (!(same(got, want) || (got != got && want != want))) fail("u_choice", b, got, want); }
                                    if (k == 0) { const double got = u0[(size_t)b * nu + j]; if (!(same(got, want) || (got != got && want != want))) fail("u0_choice", b, got, want); }
                                    ++checked;
                                }
                    }
    /* the edges of sel_source by name */
    int row = -7;
    if (sel_source(-1, 1, 3, row) != SEL_FROM_NONE || sel_source(0, 1, 3, row) != SEL_FROM_PLAN || sel_source(0, 0, 3, row) != SEL_FROM_SEQ || row != 0 ||
        sel_source(1, 1, 3, row) != SEL_FROM_SEQ || row != 0 || sel_source(2, 1, 3, row) != SEL_FROM_SEQ || row != 1 || sel_source(3, 1, 3, row) != SEL_FROM_POLICY ||
        sel_source(0, 0, 0, row) != SEL_FROM_POLICY || sel_source(0, 1, 1, row) != SEL_FROM_PLAN || sel_source(1, 1, 1, row) != SEL_FROM_POLICY) { printf("FAIL sel_source\n"); ++failures; }
    if (!sel_policy_row0(0, 1) || sel_policy_row0(1, 1) || !sel_policy_row0(2, 3) || sel_policy_row0(3, 3)) { printf("FAIL sel_policy_row0\n"); ++failures; }
    printf("chosen inputs: %d elements as the naive restatement gives them\n", checked);
}

int main()
{
    pass_through_is_open_loop();
    table_index();
    select_inputs();
    printf(failures ? "%d FAILURES\n" : "select_policy_host_check: the pass-through table is the open loop, bit for bit; every index as restated\n", failures);
    return failures ? 1 : 0;
}
