// The KPI variant of the rollout's per-trajectory core (ro_run<POLICY, true>, pyhybridcontrol_amd/csrc/rollout.inc) on the CPU: with SM_HOST a "wave" is one
// lane and the LDS block plain memory, so the evaluation in step 5 and the accumulators behind x_{k+1} run under the host sanitizers.  The hand-made one-tank
// model of scripts/rollout_host_check.cpp and the thermostat of scripts/policy_host_check.cpp.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/rollout_kpi_host_check.cpp -o /tmp/rollout_kpi_host_check && /tmp/rollout_kpi_host_check
//
// Every buffer is exactly as long as the core may use (the staging ro_stage_doubles with n_kpi, the weights rows x n_kpi, the prices K x n_chan, every
// output n_kpi), so the sanitizer sees an access past any of them.  What is expected: the statistics of the log route's own functions (ls_functional,
// ls_priced, ls_accumulate on plain arrays) over the trajectory the same call wrote out, equal in every bit, and a few figures written out by hand.
#define SM_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mldgpu.h"
#include "rollout.inc"

static int failures = 0;
static void expect(bool ok, const char *what, int k, double got, double want)
{
    if (ok) return;
    printf("FAIL %s[%d]: got %.17g, expected %.17g\n", what, k, got, want);
    ++failures;
}
static bool same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

struct Kpis {      // n_kpi KPIs over the given tables, KPI-minor, and their outputs
    int nq, rows, n_chan; unsigned given;
    int width[5];
    std::vector<double> W, thresh, price, sum, min, max; std::vector<int> chan, min_step, max_step, n_above, n_changes, n_vio;
    RoKpi Q{};
    Kpis(int nq_, unsigned given_, const int w[5], int K, bool priced, int unit) : nq(nq_), rows(0), n_chan(2), given(given_)
    {
        for (int t = 0; t < 5; ++t) { width[t] = w[t]; if (given >> t & 1u) rows += w[t]; }
        W.resize((size_t)rows * nq); thresh.resize(nq); chan.resize(nq);
        for (int r = 0; r < rows; ++r) for (int q = 0; q < nq; ++q) W[(size_t)r * nq + q] = (double)((q * 7 + r * 3) % 9 - 4) / 4.0;      // dyadic, some zero
        if (unit >= 0) { W.assign(W.size(), 0.0); W[(size_t)unit * nq] = 1.0; }                                                             // (KPI 0 = one entry of the record)
        for (int q = 0; q < nq; ++q) { thresh[q] = (double)(q % 4) - 1.0; chan[q] = priced ? q % 3 - 1 : -1; }
        if (priced) { price.resize((size_t)K * n_chan); for (size_t i = 0; i < price.size(); ++i) price[i] = 0.25 * (double)(i % 5) - 0.25; }
        sum.assign(nq, -7.0); min.assign(nq, -7.0); max.assign(nq, -7.0);
        min_step.assign(nq, -7); max_step.assign(nq, -7); n_above.assign(nq, -7); n_changes.assign(nq, -7); n_vio.assign(1, -7);
        Q.n_kpi = nq; Q.n_chan = n_chan; Q.given = given; Q.W = W.data(); Q.thresh = thresh.data(); Q.price_chan = chan.data();
        Q.price = priced ? price.data() : nullptr; Q.vio_tol = 1e-6;
        Q.sum = sum.data(); Q.min = min.data(); Q.max = max.data(); Q.min_step = min_step.data(); Q.max_step = max_step.data();
        Q.n_above = n_above.data(); Q.n_changes = n_changes.data(); Q.n_vio = n_vio.data();
    }
    // the log route's functions over the written-out trajectory (om: K x nw, vio: K), compared with what ro_run wrote
    void check(const char *name, int K, const double *x, const double *v, const double *y, const double *om, const double *vio, bool complete)
    {
        for (int q = 0; q < nq; ++q) {
            LsAcc c; ls_acc_init(c);
            for (int k = 0; k < K && complete; ++k) {
                const double *w[5]; const double *field[5] = {x + (size_t)k * width[0], v + (size_t)k * width[1], y + (size_t)k * width[2], om + (size_t)k * width[3], x + (size_t)(k + 1) * width[0]};
                int row = 0;
                for (int t = 0; t < 5; ++t) { w[t] = (given >> t & 1u) ? W.data() + (size_t)row * nq + q : nullptr; if (given >> t & 1u) row += width[t]; }
                double f = ls_functional(w, (size_t)nq, field, width);
                if (chan[q] >= 0) f = ls_priced(price[(size_t)k * n_chan + chan[q]], f);
                ls_accumulate(c, f, thresh[q], k);
            }
            const double qn = __builtin_nan("");
            expect(same(sum[q], complete ? c.sum : qn), name, q, sum[q], c.sum);
            expect(same(min[q], complete ? c.min : qn) && min_step[q] == (complete ? c.min_step : -1), name, q, min[q], c.min);
            expect(same(max[q], complete ? c.max : qn) && max_step[q] == (complete ? c.max_step : -1), name, q, max[q], c.max);
            expect(n_above[q] == (complete ? c.n_above : -1) && n_changes[q] == (complete ? c.n_changes : -1), name, q, n_above[q], c.n_above);
        }
        int nv_ = 0;
        for (int k = 0; k < K; ++k) nv_ += vio[k] > 1e-6;
        expect(n_vio[0] == (complete ? nv_ : -1), "n_vio", 0, n_vio[0], nv_);
    }
};

int main()
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
    const int width[5] = {nx, nv, ny, nw, nx};
    const double pt_u[4] = {3, 1, 4, 1}, pt_om[4] = {1, 2, 0.5, 0}, ones[8] = {1, 1, 1, 1, 1, 1, 1, 1}, junk[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    const double tab[6] = {1, 2, 5, 4, 0, 1};      // the thermostat: on (4) at x <= 2, off (0) at x >= 5

    for (int policy = 0; policy < 2; ++policy)
        for (int nq : {1, 64})
            for (int K : {1, policy ? 8 : 4})
                for (int variant = 0; variant < 2; ++variant) {      // 1: no pivot allowed, declined at step 0: NaN / -1
                    SmShape S{};
                    S.n = n; S.m = m; S.ld = n | 1; S.nb = 1; S.nx = nx; S.nW = nw + nu; S.cp = 1; S.cshift = 0;
                    S.max_nodes = 100; S.max_pivots = variant ? 0 : 1000; S.gap_abs = 1e-9; S.gap_rel = 0.0;
                    S.wave_doubles = (int)sm_wave_doubles(n, m, 1);
                    RoModel M{};
                    M.nx = nx; M.nu = nu; M.nw = nw; M.nv = nv; M.nmu = nmu; M.ny = ny; M.nc = nc; M.m = m; M.n = n;
                    M.P = PlantMats{A, B4, b5, C, D4, d5, E, F4, f5, Gy, Bv, Dv, Fv.data()};
                    M.Hx = Hx.data(); M.Hw = Hw.data(); M.H5 = H5.data(); M.rs = rs.data();
                    std::vector<double> ptab(tab, tab + 6);
                    M.pol = ptab.data();
                    SmArgs Aa{};
                    Aa.G = G.data(); Aa.q = q; Aa.lb = lb; Aa.ub = ub; Aa.cs = cs; Aa.is_int = is_int; Aa.bins = bins;
                    Kpis kp(nq, nq == 1 ? 2u : 31u, width, K, nq != 1, nq == 1 ? (policy ? 0 : 2) : -1);      // (one KPI: w_v = e_z, under the policy e_u)
                    std::vector<double> mem((size_t)S.wave_doubles), stg(ro_stage_doubles(nx, nu, nw, m, nv, ny, nq));
                    std::vector<double> x((size_t)(K + 1) * nx, -7.0), v((size_t)K * nv, -7.0), y((size_t)K * ny, -7.0), vio(K, -7.0);
                    std::vector<double> u(policy ? junk : pt_u, (policy ? junk : pt_u) + K), om(policy ? ones : pt_om, (policy ? ones : pt_om) + K), up(1, 0.0);
                    const double x0 = policy ? 3.0 : 2.0;
                    RoTraj T{};
                    T.K = K; T.x0 = &x0; T.u = u.data(); T.u_step = nu; T.om = om.data(); T.x = x.data(); T.v = v.data(); T.y = y.data(); T.vio = vio.data(); T.u_prev = up.data();
                    RoResult R{};
                    if (policy) ro_run<true, true>(S, M, mem.data(), stg.data(), Aa, T, 0, R, &kp.Q);
                    else ro_run<false, true>(S, M, mem.data(), stg.data(), Aa, T, 0, R, &kp.Q);
                    expect(R.end_status == (variant ? RO_DECLINED : RO_COMPLETE), "end_status", variant, R.end_status, variant ? RO_DECLINED : RO_COMPLETE);
                    kp.check(policy ? "policy KPIs" : "open-loop KPIs", K, x.data(), v.data(), y.data(), om.data(), vio.data(), !variant);
                    if (nq == 1 && !variant && K > 1) {      // by hand: the realised import z = 2, 0, 3.5, 1 (the solver's z to 1e-9); the thermostat's u = 0, 4, 4, 0, 0, 0, 4, 4 (exact)
                        if (!policy) expect(fabs(kp.sum[0] - 6.5) <= 1e-9 && fabs(kp.max[0] - 3.5) <= 1e-9 && kp.max_step[0] == 2 && fabs(kp.min[0]) <= 1e-9 && kp.min_step[0] == 1 && kp.n_vio[0] == 1, "sum z", 0, kp.sum[0], 6.5);
                        else expect(kp.sum[0] == 16.0 && kp.n_changes[0] == 3 && kp.n_changes[0] == R.switches && kp.max_step[0] == 1 && kp.min_step[0] == 0, "sum u, switches", 0, kp.sum[0], 16.0);
                    }
                    printf("policy %d, n_kpi %2d, K %d, variant %d: end_status %d, sum[0] %g, n_vio %d\n", policy, nq, K, variant, R.end_status, kp.sum[0], kp.n_vio[0]);
                }
    // a tabled model without auxiliaries (n = 0, no output, no rows): x+ = 0.5 x + u + 0.5 under the thermostat; the record has no y
    for (int nq : {1, 64})
        for (int K : {1, 3}) {
            const double A1[1] = {0.5}, B41[1] = {0}, b51[1] = {0.5}, Bv1[1] = {1}, x0 = 1.0;
            const int w1[5] = {1, 1, 0, 1, 1};
            RoModel M{};
            M.nx = 1; M.nu = 1; M.nw = 1; M.nv = 1; M.P.A = A1; M.P.B4 = B41; M.P.b5 = b51; M.P.Bv = Bv1;
            std::vector<double> ptab(tab, tab + 6);
            M.pol = ptab.data();
            SmShape S{}; SmArgs Aa{};
            Kpis kp(nq, nq == 1 ? 2u : 27u, w1, K, nq != 1, nq == 1 ? 0 : -1);      // (x, v, omega, x_k1: a table of y would be refused by the host; one KPI: w_v = e_u)
            std::vector<double> stg(ro_stage_doubles(1, 1, 1, 0, 1, 0, nq)), x(K + 1), v(K), vio(K), u(junk, junk + K), om(K, 0.0), up(1, 0.0), y(1);
            RoTraj T{};
            T.K = K; T.x0 = &x0; T.u = u.data(); T.u_step = 1; T.om = om.data(); T.x = x.data(); T.v = v.data(); T.vio = vio.data(); T.u_prev = up.data();
            RoResult R{};
            ro_run<true, true>(S, M, nullptr, stg.data(), Aa, T, 0, R, &kp.Q);
            expect(R.end_status == RO_COMPLETE, "tabled end_status", K, R.end_status, RO_COMPLETE);
            kp.check("tabled KPIs", K, x.data(), v.data(), y.data(), om.data(), vio.data(), true);
            if (nq == 1 && K == 3) expect(kp.sum[0] == 4.0 && kp.n_changes[0] == 1 && kp.n_vio[0] == 0, "tabled sum u", 0, kp.sum[0], 4.0);      // x: 1, 5, 3 -> u: 4, 0, 0
            printf("tabled, n_kpi %2d, K %d: sum[0] %g, n_changes[0] %d\n", nq, K, kp.sum[0], kp.n_changes[0]);
        }
    printf(failures ? "%d FAILURES\n" : "rollout_kpi_host_check: every statistic as the log route's functions give it\n", failures);
    return failures ? 1 : 0;
}
