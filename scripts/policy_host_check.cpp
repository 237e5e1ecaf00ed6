// The policy instantiation of k_rollout_policy's per-trajectory core (ro_run<true>, pyhybridcontrol_amd/csrc/rollout.inc) on the CPU: with SM_HOST a
// "wave" is one lane and the LDS block plain memory, so the feedback rule inside the loop over k runs under the host sanitizers.  The hand-made one-tank
// model of scripts/rollout_host_check.cpp, every value below worked out by hand.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/policy_host_check.cpp -o /tmp/policy_host_check && /tmp/policy_host_check
//
// The model (nx = nu = nomega = ndelta = nz = nmu = ny = 1): p = u - omega is the net power, delta = [p >= 0] and z = delta p by six big-M rows (M = 10),
// the tank x+ = 0.5 x + z + 0.5 with the soft bound x - mu <= 4 and y = x + z; v = [u; delta; z; mu].  The thermostat: on (u = 4) at x <= 2, off (u = 0)
// at x >= 5, in between what it was; omega = 1 throughout, so that on means x+ = 0.5 x + 3.5 and off x+ = 0.5 x + 0.5.
#define SM_HOST
#include <stdio.h>
#include <stdlib.h>
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

struct Case {
    const char *name;
    int K;
    double x0, u_prev;
    double tab[6];                  // [sel | on_at | off_at | u_on | u_off | mode]
    const double *u_seq, *om_seq;   // K each
    const double *want_x, *want_v;  // K + 1, K x 4
    int want_switches;
};

int main()
{
    const double BM = 10.0;
    const int nx = 1, nu = 1, nw = 1, nv = 4, nmu = 1, ny = 1, n = 3, m = 7, nc = 7;
    // rows:            p <= M d        -p <= M (1 - d)   z <= M d     -z <= 0      z <= p + M (1 - d)   z >= p - M (1 - d)   x - mu <= 4
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

    const double ones[8] = {1, 1, 1, 1, 1, 1, 1, 1}, junk[8] = {9, 9, 9, 9, 9, 9, 9, 9};      // a ruled channel never reads u_seq
    // a tank that cycles: off inside the band, on at x == 2 EXACTLY (the tie of the first line), holds, off above 5, on again below 2
    const double cyc_x[9] = {3, 2, 4.5, 5.75, 3.375, 2.1875, 1.59375, 4.296875, 5.6484375};
    const double cyc_v[32] = {0, 0, 0, 0,  4, 1, 3, 0,  4, 1, 3, 0.5,  0, 0, 0, 1.75,  0, 0, 0, 0,  0, 0, 0, 0,  4, 1, 3, 0,  4, 1, 3, 0.296875};
    // the tie of the second line: x == off_at EXACTLY while on
    const double off_x[2] = {5, 3}, off_v[4] = {0, 0, 0, 1};
    // strictly inside while on: holds, no switch
    const double in_x[2] = {3, 5}, in_v[4] = {4, 1, 3, 0};
    // on_at == off_at == x: the first line wins
    const double eq_x[2] = {3, 5}, eq_v[4] = {4, 1, 3, 0};
    // the channel passed through (mode 0): rollout_host_check's own trajectory, from u_seq
    const double pt_u[4] = {3, 1, 4, 1}, pt_om[4] = {1, 2, 0.5, 0}, pt_x[5] = {2, 3.5, 2.25, 5.125, 4.0625};
    const double pt_v[16] = {3, 1, 2, 0, 1, 0, 0, 0, 4, 1, 3.5, 0, 1, 1, 1, 1.125};
    const Case cases[] = {
        {"a tank that cycles", 8, 3.0, 0.0, {1, 2, 5, 4, 0, 1}, junk, ones, cyc_x, cyc_v, 3},
        {"x == off_at while on", 1, 5.0, 4.0, {1, 2, 5, 4, 0, 1}, junk, ones, off_x, off_v, 1},
        {"inside the band while on", 1, 3.0, 4.0, {1, 2, 5, 4, 0, 1}, junk, ones, in_x, in_v, 0},
        {"on_at == off_at == x", 1, 3.0, 0.0, {1, 3, 3, 4, 0, 1}, junk, ones, eq_x, eq_v, 1},
        {"a passed-through channel", 4, 2.0, 7.0, {1, 2, 5, 4, 0, 0}, pt_u, pt_om, pt_x, pt_v, 0},
    };
    for (const Case &c : cases) {
        const int K = c.K;
        SmShape S{};
        S.n = n; S.m = m; S.ld = n | 1; S.nb = 1; S.nx = nx; S.nW = nw + nu; S.cp = 1; S.cshift = 0;
        S.max_nodes = 100; S.max_pivots = 1000; S.gap_abs = 1e-9; S.gap_rel = 0.0;
        S.wave_doubles = (int)sm_wave_doubles(n, m, 1);
        RoModel M{};
        M.nx = nx; M.nu = nu; M.nw = nw; M.nv = nv; M.nmu = nmu; M.ny = ny; M.nc = nc; M.m = m; M.n = n;
        M.P = PlantMats{A, B4, b5, C, D4, d5, E, F4, f5, Gy, Bv, Dv, Fv.data()};
        M.Hx = Hx.data(); M.Hw = Hw.data(); M.H5 = H5.data(); M.rs = rs.data();
        std::vector<double> tab(c.tab, c.tab + 6);      // exactly nu (nx + 5) doubles: the sanitizer sees a read past the table
        M.pol = tab.data();
        SmArgs Aa{};
        Aa.G = G.data(); Aa.q = q; Aa.lb = lb; Aa.ub = ub; Aa.cs = cs; Aa.is_int = is_int; Aa.bins = bins;
        // exactly the doubles the core may use: the staging is ro_stage_doubles, as without a policy (u_{k-1} lives in v's block)
        std::vector<double> mem((size_t)S.wave_doubles), stg(ro_stage_doubles(nx, nu, nw, m, nv, ny));
        std::vector<double> x((size_t)(K + 1) * nx, -7.0), v((size_t)K * nv, -7.0), y((size_t)K * ny, -7.0), u(c.u_seq, c.u_seq + K), om(c.om_seq, c.om_seq + K), up(1, c.u_prev);
        RoTraj T{};
        T.K = K; T.x0 = &c.x0; T.u = u.data(); T.u_step = nu; T.om = om.data(); T.x = x.data(); T.v = v.data(); T.y = y.data(); T.u_prev = up.data();
        RoResult R{};
        R.switches = -7;
        ro_run<true>(S, M, mem.data(), stg.data(), Aa, T, 0, R);
        expect(R.end_status == RO_COMPLETE && R.steps_done == K, c.name, 0, R.end_status, RO_COMPLETE);
        expect(R.switches == c.want_switches, "switches", 0, R.switches, c.want_switches);
        double mu_total = 0.0;
        for (int k = 0; k <= K; ++k) expect(x[k] == c.want_x[k], "x", k, x[k], c.want_x[k]);      // (dyadic values: the sums are exact)
        for (int k = 0; k < K; ++k) {
            for (int j = 0; j < nv; ++j) expect(j == 0 ? v[k * nv] == c.want_v[k * nv] : fabs(v[k * nv + j] - c.want_v[k * nv + j]) <= 1e-9, "v", k * nv + j, v[k * nv + j], c.want_v[k * nv + j]);
            expect(fabs(y[k] - (c.want_x[k] + c.want_v[k * nv + 2])) <= 1e-9, "y", k, y[k], c.want_x[k] + c.want_v[k * nv + 2]);
            mu_total += c.want_v[k * nv + 3];
        }
        expect(fabs(R.mu_total - mu_total) <= 1e-9, "mu_total", 0, R.mu_total, mu_total);
        printf("%s: end_status %d, steps_done %d, switches %d\n", c.name, R.end_status, R.steps_done, R.switches);
    }
    // the open-loop instantiation leaves the policy's fields alone
    {
        const double A1[1] = {0.5}, B41[1] = {0}, b51[1] = {0.5}, Bv1[1] = {1}, u[2] = {1, 2}, om[2] = {0, 0}, x0[1] = {2};
        RoModel M{};
        M.nx = 1; M.nu = 1; M.nw = 1; M.nv = 1; M.P.A = A1; M.P.B4 = B41; M.P.b5 = b51; M.P.Bv = Bv1;
        SmShape S{}; SmArgs Aa{};
        std::vector<double> stg(ro_stage_doubles(1, 1, 1, 0, 1, 0)), x(3);
        RoTraj T{};
        T.K = 2; T.x0 = x0; T.u = u; T.u_step = 1; T.om = om; T.x = x.data();
        RoResult R{};
        R.switches = -7;
        ro_run(S, M, nullptr, stg.data(), Aa, T, 0, R);
        expect(x[2] == 3.75 && R.switches == -7 && R.end_status == RO_COMPLETE, "open loop", 0, x[2], 3.75);
    }
    printf(failures ? "%d FAILURES\n" : "policy_host_check: all values as written out\n", failures);
    return failures ? 1 : 0;
}
