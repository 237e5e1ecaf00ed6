// The per-trajectory core of k_rollout (ro_run, pyhybridcontrol_amd/csrc/rollout.inc) on the CPU: with SM_HOST a "wave" is one lane and the LDS block plain
// memory, so the loop over k around sm_solve runs under the host sanitizers.  A hand-made one-tank model with unit scales, four steps, every value below
// worked out by hand.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/rollout_host_check.cpp -o /tmp/rollout_host_check && /tmp/rollout_host_check
//
// The model (nx = nu = nomega = ndelta = nz = nmu = ny = 1): p = u - omega is the net power, delta = [p >= 0] and z = delta p by six big-M rows (M = 10),
// the tank x+ = 0.5 x + z + 0.5 with the soft bound x - mu <= 4 and y = x + z; v = [u; delta; z; mu].  The hard variant adds the row x <= 5.
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
static bool near(double a, double b) { return fabs(a - b) <= 1e-9; }

int main()
{
    const double BM = 10.0;
    const int nx = 1, nu = 1, nw = 1, nv = 4, nmu = 1, ny = 1, n = 3, K = 4;
    // rows:            p <= M d        -p <= M (1 - d)   z <= M d     -z <= 0      z <= p + M (1 - d)   z >= p - M (1 - d)   x - mu <= 4    x <= 5 (hard variant)
    const double E[8] = {0, 0, 0, 0, 0, 0, 1, 1}, F1[8] = {1, -1, 0, 0, -1, 1, 0, 0}, F2[8] = {-BM, BM, -BM, 0, BM, BM, 0, 0}, F3[8] = {0, 0, 1, -1, 1, -1, 0, 0};
    const double F4[8] = {-1, 1, 0, 0, 1, -1, 0, 0}, Psi[8] = {0, 0, 0, 0, 0, 0, -1, 0}, f5[8] = {0, BM, 0, 0, BM, BM, 4, 5}, Gy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const double A[1] = {0.5}, B4[1] = {0}, b5[1] = {0.5}, C[1] = {1}, D4[1] = {0}, d5[1] = {0};
    const double Bv[4] = {0, 0, 1, 0}, Dv[4] = {0, 0, 1, 0};
    const double u_seq[K] = {3, 1, 4, 1}, om_seq[K] = {1, 2, 0.5, 0}, x0[1] = {2};
    const double cw[K * 4] = {1, 0, 2, 0.5, 1, 0, 2, 0.5, 1, 0, 2, 0.5, 1, 0, 2, 0.5};
    // what the four steps are
    const double want_x[K + 1] = {2, 3.5, 2.25, 5.125, 4.0625}, want_y[K] = {4, 3.5, 5.75, 6.125};
    const double want_v[K * 4] = {3, 1, 2, 0, 1, 0, 0, 0, 4, 1, 3.5, 0, 1, 1, 1, 1.125};
    const double want_vio[K] = {0, 0, 0, 1.125}; const int want_row[K] = {4, 2, 4, 6};

    for (int variant = 0; variant < 3; ++variant) {      // 0: the soft model; 1: with the hard row, infeasible at step 3; 2: no pivots allowed, declined at step 0
        const int m = variant == 1 ? 8 : 7, nc = m;
        std::vector<double> Fv((size_t)nc * nv), G((size_t)m * n), Hx(m), Hw((size_t)m * 2), H5(m), rs(m, 1.0);
        for (int i = 0; i < m; ++i) {
            Fv[i * nv + 0] = F1[i]; Fv[i * nv + 1] = F2[i]; Fv[i * nv + 2] = F3[i]; Fv[i * nv + 3] = Psi[i];
            G[i * n + 0] = F2[i]; G[i * n + 1] = F3[i]; G[i * n + 2] = Psi[i];            // the rows in the unknowns [delta, z, mu] (G y adds nothing: Gy = 0)
            Hx[i] = -E[i]; Hw[i * 2 + 0] = -F4[i]; Hw[i * 2 + 1] = -F1[i]; H5[i] = f5[i];    // h = f5 - E x - F4 omega - F1 u, omega' = [omega; u]
        }
        const double q[3] = {0, 0, 1}, lb[3] = {0, -BM, 0}, ub[3] = {1, BM, S_INF}, cs[3] = {1, 1, 1};
        const unsigned char is_int[3] = {1, 0, 0}; const int bins[1] = {0};
        SmShape S{};
        S.n = n; S.m = m; S.ld = n | 1; S.nb = 1; S.nx = nx; S.nW = nw + nu; S.cp = 1; S.cshift = 0;      // (one lane: one lane across a dictionary row)
        S.max_nodes = 100; S.max_pivots = variant == 2 ? 0 : 1000; S.gap_abs = 1e-9; S.gap_rel = 0.0;
        S.wave_doubles = (int)sm_wave_doubles(n, m, 1);
        RoModel M{};
        M.nx = nx; M.nu = nu; M.nw = nw; M.nv = nv; M.nmu = nmu; M.ny = ny; M.nc = nc; M.m = m; M.n = n;
        M.P = PlantMats{A, B4, b5, C, D4, d5, E, F4, f5, Gy, Bv, Dv, Fv.data()};
        M.Hx = Hx.data(); M.Hw = Hw.data(); M.H5 = H5.data(); M.rs = rs.data();
        SmArgs Aa{};
        Aa.G = G.data(); Aa.q = q; Aa.lb = lb; Aa.ub = ub; Aa.cs = cs; Aa.is_int = is_int; Aa.bins = bins;
        // exactly the doubles the core may use: the sanitizer sees every access past either block
        std::vector<double> mem((size_t)S.wave_doubles), stg(ro_stage_doubles(nx, nu, nw, m, nv, ny));
        std::vector<double> x((size_t)(K + 1) * nx, -7.0), v((size_t)K * nv, -7.0), y((size_t)K * ny, -7.0), vio(K, -7.0); std::vector<int> row(K, -7);
        RoTraj T{};
        T.K = K; T.x0 = x0; T.u = u_seq; T.u_step = nu; T.om = om_seq; T.cw = cw; T.x = x.data(); T.v = v.data(); T.y = y.data(); T.vio = vio.data(); T.row = row.data();
        RoResult R{};
        ro_run(S, M, mem.data(), stg.data(), Aa, T, 0, R);
        const int done = variant == 0 ? K : (variant == 1 ? 3 : 0), end = variant == 0 ? RO_COMPLETE : (variant == 1 ? RO_INFEASIBLE : RO_DECLINED);
        expect(R.end_status == end, "end_status", variant, R.end_status, end);
        expect(R.steps_done == done, "steps_done", variant, R.steps_done, done);
        for (int k = 0; k <= K; ++k) expect(k <= done ? near(x[k], want_x[k]) : x[k] != x[k], "x", k, x[k], want_x[k]);
        for (int k = 0; k < K; ++k) {
            const bool live = k < done;
            for (int j = 0; j < nv; ++j) expect(live ? near(v[k * nv + j], want_v[k * nv + j]) : v[k * nv + j] != v[k * nv + j], "v", k * nv + j, v[k * nv + j], want_v[k * nv + j]);
            expect(live ? near(y[k], want_y[k]) : y[k] != y[k], "y", k, y[k], want_y[k]);
            expect(live ? near(vio[k], want_vio[k]) : vio[k] != vio[k], "cons_vio", k, vio[k], want_vio[k]);
            expect(row[k] == (live ? want_row[k] : -1), "cons_row", k, row[k], live ? want_row[k] : -1);
        }
        if (variant == 0) {
            expect(near(R.cost, 22.5625), "cost", 0, R.cost, 22.5625);
            expect(near(R.mu_total, 1.125), "mu_total", 0, R.mu_total, 1.125);
            expect(near(R.worst_vio, 1.125) && R.worst_step == 3 && R.worst_row == 6, "worst_vio", R.worst_step, R.worst_vio, 1.125);
        } else {
            expect(R.cost != R.cost && R.mu_total != R.mu_total && R.worst_vio != R.worst_vio && R.worst_step == -1, "summaries of an unfinished trajectory", variant, R.cost, NAN);
        }
        printf("variant %d: end_status %d, steps_done %d\n", variant, R.end_status, R.steps_done);
    }
    // without auxiliaries (n = 0) the rollout is a plain lsim: x+ = 0.5 x + u + 0.5, no rows
    {
        const double A[1] = {0.5}, B4[1] = {0}, b5[1] = {0.5}, Bv[1] = {1}, u[3] = {1, 2, 3}, om[3] = {0, 0, 0}, x0[1] = {2};
        RoModel M{};
        M.nx = 1; M.nu = 1; M.nw = 1; M.nv = 1; M.P.A = A; M.P.B4 = B4; M.P.b5 = b5; M.P.Bv = Bv;
        SmShape S{}; SmArgs Aa{};
        std::vector<double> stg(ro_stage_doubles(1, 1, 1, 0, 1, 0)), x(4), vio(3); std::vector<int> row(3);
        RoTraj T{};
        T.K = 3; T.x0 = x0; T.u = u; T.u_step = 1; T.om = om; T.x = x.data(); T.vio = vio.data(); T.row = row.data();
        RoResult R{};
        ro_run(S, M, nullptr, stg.data(), Aa, T, 0, R);
        const double want[4] = {2, 2.5, 3.75, 5.375};
        for (int k = 0; k < 4; ++k) expect(x[k] == want[k], "plain x", k, x[k], want[k]);
        expect(R.end_status == RO_COMPLETE && R.steps_done == 3 && R.worst_vio == -S_INF && R.worst_step == 0 && row[2] == -1 && R.cost == 0.0 && R.mu_total == 0.0, "plain summary", 0, R.worst_vio, -S_INF);
    }
    printf(failures ? "%d FAILURES\n" : "rollout_host_check: all values as written out\n", failures);
    return failures ? 1 : 0;
}
