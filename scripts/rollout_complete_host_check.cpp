// What the device completion of declined trajectories adds to the rollout body (pyhybridcontrol_amd/csrc/rollout.inc: ro_run's third flag, FIX), on the CPU
// under the host sanitizers: with SM_HOST a "wave" is one lane and the LDS block plain memory.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/rollout_complete_host_check.cpp -o /tmp/rollout_complete_host_check && /tmp/rollout_complete_host_check
//
// The one-tank model of scripts/policy_host_check.cpp.  The table, the marks, the slot's input rows and the step are each exactly as long as the rule allows
// ro_run to touch (K n, K, nx, nw + nu, 1), so that the sanitizer sees an access past them.
// 1. An empty table and a full budget: ro_run<., ., true> is ro_run<., ., false>, bit for bit, and reports step -1.
// 2. A decline with the table empty (pivot budget 2): the trajectory ends 2 at the first declined step k, step == k, and the slot holds x_k and
//    [omega_k; u_k] of the reference run, bit for bit.
// 3. The rounds of the rule: every declined step answered with the reference run's delta, z, mu until the trajectory ends 0 -- at most K rounds and one
//    more run -- and then every output equals the reference run's, bit for bit.
// 4. A fix at step 0 alone and at step K - 1 alone (full budget elsewhere): the reference run again.
// 5. A "no feasible point" mark at step 0, in the middle and at step K - 1: the trajectory ends 1 there, NaN / -1 from there on, step -1.
// Open loop (the pass-through table under POLICY = true, as k_rollout_redo runs it) and the thermostat in closed loop.
#define SM_HOST
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mldgpu.h"
#include "rollout.inc"

static int failures = 0;
static void fail(const char *what, long long i, double got, double want)
{
    printf("FAIL %s[%lld]: got %.17g, expected %.17g\n", what, i, got, want);
    ++failures;
}

enum { NX = 1, NU = 1, NW = 1, NV = 4, NMU = 1, NY = 1, N = 3, M_ROWS = 7, NC = 7, K = 6 };

struct Model {
    std::vector<double> Fv, G, Hx, Hw, H5, rs, tab;
    RoModel M{};
    SmArgs A{};
    SmShape S{};
};
struct Out {
    std::vector<double> x, v, y, vio; std::vector<int> row; RoResult R{};
    bool operator==(const Out &o) const
    {
        return !memcmp(x.data(), o.x.data(), sizeof(double) * x.size()) && !memcmp(v.data(), o.v.data(), sizeof(double) * v.size()) &&
               !memcmp(y.data(), o.y.data(), sizeof(double) * y.size()) && !memcmp(vio.data(), o.vio.data(), sizeof(double) * vio.size()) && row == o.row &&
               !memcmp(&R.cost, &o.R.cost, sizeof(double)) && !memcmp(&R.mu_total, &o.R.mu_total, sizeof(double)) && !memcmp(&R.worst_vio, &o.R.worst_vio, sizeof(double)) &&
               R.worst_step == o.R.worst_step && R.worst_row == o.R.worst_row && R.steps_done == o.R.steps_done && R.end_status == o.R.end_status && R.switches == o.R.switches;
    }
};

static const double BM = 10.0;
static const double E_[7] = {0, 0, 0, 0, 0, 0, 1}, F1[7] = {1, -1, 0, 0, -1, 1, 0}, F2[7] = {-BM, BM, -BM, 0, BM, BM, 0}, F3[7] = {0, 0, 1, -1, 1, -1, 0};
static const double F4[7] = {-1, 1, 0, 0, 1, -1, 0}, Psi[7] = {0, 0, 0, 0, 0, 0, -1}, f5[7] = {0, BM, 0, 0, BM, BM, 4}, Gy[7] = {0, 0, 0, 0, 0, 0, 0};
static const double A_[1] = {0.5}, B4[1] = {0}, b5[1] = {0.5}, C_[1] = {1}, D4[1] = {0}, d5[1] = {0}, Bv[4] = {0, 0, 1, 0}, Dv[4] = {0, 0, 1, 0};
static const double q_[3] = {0, 0, 1}, lb_[3] = {0, -BM, 0}, ub_[3] = {1, BM, S_INF}, cs_[3] = {1, 1, 1};
static const unsigned char is_int_[3] = {1, 0, 0};
static const int bins_[1] = {0};

static void build(Model &o, bool ruled, int max_pivots)
{
    o.Fv.assign((size_t)NC * NV, 0.0); o.G.assign((size_t)M_ROWS * N, 0.0); o.Hx.assign(M_ROWS, 0.0); o.Hw.assign((size_t)M_ROWS * 2, 0.0); o.H5.assign(M_ROWS, 0.0);
    o.rs.assign(M_ROWS, 1.0);
    for (int i = 0; i < M_ROWS; ++i) {
        o.Fv[i * NV + 0] = F1[i]; o.Fv[i * NV + 1] = F2[i]; o.Fv[i * NV + 2] = F3[i]; o.Fv[i * NV + 3] = Psi[i];
        o.G[i * N + 0] = F2[i]; o.G[i * N + 1] = F3[i]; o.G[i * N + 2] = Psi[i];
        o.Hx[i] = -E_[i]; o.Hw[i * 2 + 0] = -F4[i]; o.Hw[i * 2 + 1] = -F1[i]; o.H5[i] = f5[i];
    }
    o.tab.assign((size_t)NU * (NX + POL_TAIL), 0.0);      /* all zero: every channel passed through */
    if (ruled) { o.tab[0] = 1.0; o.tab[NX + POL_ON_AT] = 1.5; o.tab[NX + POL_OFF_AT] = 3.0; o.tab[NX + POL_U_ON] = 4.0; o.tab[NX + POL_U_OFF] = 0.0; o.tab[NX + POL_MODE] = 1.0; }
    o.S.n = N; o.S.m = M_ROWS; o.S.ld = N | 1; o.S.nb = 1; o.S.nx = NX; o.S.nW = NW + NU; o.S.cp = 1; o.S.cshift = 0;
    o.S.max_nodes = 100; o.S.max_pivots = max_pivots; o.S.gap_abs = 1e-9; o.S.gap_rel = 0.0;
    o.S.wave_doubles = (int)sm_wave_doubles(N, M_ROWS, 1);
    o.M.nx = NX; o.M.nu = NU; o.M.nw = NW; o.M.nv = NV; o.M.nmu = NMU; o.M.ny = NY; o.M.nc = NC; o.M.m = M_ROWS; o.M.n = N;
    o.M.P = PlantMats{A_, B4, b5, C_, D4, d5, E_, F4, f5, Gy, Bv, Dv, o.Fv.data()};
    o.M.Hx = o.Hx.data(); o.M.Hw = o.Hw.data(); o.M.H5 = o.H5.data(); o.M.rs = o.rs.data(); o.M.pol = o.tab.data();
    o.A.G = o.G.data(); o.A.q = q_; o.A.lb = lb_; o.A.ub = ub_; o.A.cs = cs_; o.A.is_int = is_int_; o.A.bins = bins_;
}

struct Fix {      /* every array exactly as long as ro_run may touch */
    std::vector<double> ans = std::vector<double>((size_t)K * N, -7.0), ax0 = std::vector<double>(NX, -7.0), aom = std::vector<double>(NW + NU, -7.0);
    std::vector<int> mark = std::vector<int>(K, RO_FIX_OPEN), step = std::vector<int>(1, -7);
    RoFix view() { RoFix F{}; F.ans = ans.data(); F.mark = mark.data(); F.ax0 = ax0.data(); F.aom = aom.data(); F.step = step.data(); return F; }
};

static const double U_SEQ[K] = {3, 1, 4, 1, 0.3, 2.7}, OM[K] = {1, 2, 0.5, 0, 1.1, 0.7};
static const double CW[K * NV] = {1, 0.5, 2, 3, 1.5, 0.25, 1, 1, 2, 2, 2, 2, 0.1, 0.2, 0.3, 0.4, 1, 0.5, 2, 3, 1.5, 0.25, 1, 1};

template <bool FIX> static Out run(const Model &o, double x0, Fix *fix)
{
    Out r;
    std::vector<double> mem((size_t)o.S.wave_doubles), stg(ro_stage_doubles(NX, NU, NW, M_ROWS, NV, NY));
    r.x.assign((size_t)(K + 1) * NX, -7.0); r.v.assign((size_t)K * NV, -7.0); r.y.assign((size_t)K * NY, -7.0); r.vio.assign(K, -7.0); r.row.assign(K, -7);
    const double up[1] = {0.0};
    RoTraj T{};
    T.K = K; T.x0 = &x0; T.u = U_SEQ; T.u_step = NU; T.om = OM; T.cw = CW;
    T.x = r.x.data(); T.v = r.v.data(); T.y = r.y.data(); T.vio = r.vio.data(); T.row = r.row.data(); T.u_prev = up;
    r.R.switches = -7;
    if constexpr (FIX) { const RoFix F = fix->view(); ro_run<true, false, true>(o.S, o.M, mem.data(), stg.data(), o.A, T, 0, r.R, nullptr, &F); }
    else ro_run<true, false, false>(o.S, o.M, mem.data(), stg.data(), o.A, T, 0, r.R);
    return r;
}

static void answer(Fix &f, const Out &ref, int k)
{
    for (int j = 0; j < N; ++j) f.ans[(size_t)k * N + j] = ref.v[(size_t)k * NV + NU + j];
    f.mark[k] = RO_FIX_ANSWER;
}

static void check_case(bool ruled, double x0, int id)
{
    Model full, capped;
    build(full, ruled, 1000); build(capped, ruled, 2);
    const Out ref = run<false>(full, x0, nullptr);
    if (ref.R.end_status != RO_COMPLETE) { fail("the reference run ends 0", id, ref.R.end_status, RO_COMPLETE); return; }
    {   /* 1 */
        Fix f;
        const Out got = run<true>(full, x0, &f);
        if (!(got == ref)) fail("empty table, full budget: the plain body", id, 0, 0);
        if (f.step[0] != -1) fail("step of a trajectory that ended 0", id, f.step[0], -1);
        if (f.ax0[0] != -7.0 || f.aom[0] != -7.0) fail("no decline: the slot is not written", id, f.ax0[0], -7.0);
    }
    int first = -1;
    {   /* 2 and 3 */
        Fix f;
        int rounds = 0;
        Out got;
        for (int r = 0; r <= K; ++r) {
            got = run<true>(capped, x0, &f);
            const int k = f.step[0];
            if (got.R.end_status != RO_DECLINED) { if (k != -1) fail("step of a finished trajectory", id, k, -1); break; }
            if (r == 0) first = k;
            if (k < r || k >= K || got.R.steps_done != k) { fail("the declining step moves forward", id, k, r); return; }
            if (f.mark[k] != RO_FIX_OPEN) fail("a decline only where the table has no answer", id, f.mark[k], RO_FIX_OPEN);
            if (memcmp(&f.ax0[0], &ref.x[(size_t)k * NX], sizeof(double))) fail("slot x_k", id, f.ax0[0], ref.x[(size_t)k * NX]);
            if (memcmp(&f.aom[0], &OM[k], sizeof(double))) fail("slot omega_k", id, f.aom[0], OM[k]);
            if (memcmp(&f.aom[NW], &ref.v[(size_t)k * NV], sizeof(double))) fail("slot u_k (the rule's under a policy)", id, f.aom[NW], ref.v[(size_t)k * NV]);
            for (int s = k; s < K; ++s) if (got.v[(size_t)s * NV] == got.v[(size_t)s * NV] || got.row[s] != -1) fail("NaN / -1 from the declined step on", id, got.v[(size_t)s * NV], 0);
            if (r == K) { fail("still declined after K rounds", id, k, -1); return; }
            answer(f, ref, k);
            ++rounds;
        }
        if (!(got == ref)) fail("after the rounds: the reference run", id, got.R.end_status, 0);
        printf("case %d (%s, x0 %.2f): first decline at step %d, %d round(s)\n", id, ruled ? "closed loop" : "open loop", x0, first, rounds);
    }
    for (int k : {0, K - 1}) {   /* 4 */
        Fix f;
        answer(f, ref, k);
        const Out got = run<true>(full, x0, &f);
        if (!(got == ref) || f.step[0] != -1) fail("a fix at one step", 10 * id + k, f.step[0], -1);
    }
    for (int k : {0, K / 2, K - 1}) {   /* 5 */
        Fix f;
        for (int s = 0; s < k; ++s) answer(f, ref, s);      /* (mixed with answers before it) */
        f.mark[k] = RO_FIX_NO_POINT;
        const Out got = run<true>(full, x0, &f);
        if (got.R.end_status != RO_INFEASIBLE || got.R.steps_done != k || f.step[0] != -1) fail("no feasible point: ends 1 at the step", 10 * id + k, got.R.steps_done, k);
        if (got.R.cost == got.R.cost || got.R.worst_step != -1 || got.R.switches != -1) fail("no feasible point: summaries NaN / -1", 10 * id + k, got.R.cost, 0);
        if (memcmp(got.x.data(), ref.x.data(), sizeof(double) * (size_t)(k + 1) * NX) || memcmp(got.v.data(), ref.v.data(), sizeof(double) * (size_t)k * NV))
            fail("no feasible point: the steps before it stay", 10 * id + k, 0, 0);
        for (int s = k; s < K; ++s)
            if (got.v[(size_t)s * NV] == got.v[(size_t)s * NV] || got.y[s] == got.y[s] || got.vio[s] == got.vio[s] || got.row[s] != -1 || got.x[(size_t)(s + 1) * NX] == got.x[(size_t)(s + 1) * NX])
                fail("no feasible point: NaN / -1 from there on", 10 * id + s, got.v[(size_t)s * NV], 0);
    }
}

int main()
{
    int id = 0;
    for (int ruled = 0; ruled <= 1; ++ruled)
        for (double x0 : {2.0, 2.75, 3.5, 0.25}) check_case(ruled != 0, x0, id++);
    printf(failures ? "%d FAILURES\n" : "rollout_complete_host_check: table, marks, slot and step as the rule states them, bit for bit\n", failures);
    return failures ? 1 : 0;
}
