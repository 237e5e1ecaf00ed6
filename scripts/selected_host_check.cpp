// The rules of the selected step (sel_step_source, sel_step_input, sel_step_pick, sel_step_remembered, sel_step_next_age, sel_kept_policy,
// pyhybridcontrol_amd/csrc/selected.inc) on the CPU: the per-element bodies of k_selected_inputs and k_selected_commit are host-compilable functions (SM_HOST,
// as fallback.inc), so the loops the kernels run per (instance, channel) and per memory element run here under the host sanitizers, every array sized to the
// byte -- sel_u of an instance has exactly K nu doubles, its memory exactly N nu, so a read past a row of either is seen.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/selected_host_check.cpp -o /tmp/selected_host_check && /tmp/selected_host_check
//
// Part 1, the index edges: choice -1 / 0 / 63, policy -1 / 0, age -1 / 1 / N - 1 / N, K 1 / N - 1 / N, every fb, against a restatement written out as a table.
// Part 2, the example of tests/test_selected_host.py, every value worked out by hand.
#define SM_HOST
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "mldgpu.h"
#include "rollout.inc"
#include "fallback.inc"
#include "selected.inc"

static int failures = 0;
static void expect(bool ok, const char *what, int a, int b, double got, double want)
{
    if (ok) return;
    printf("FAIL %s[%d, %d]: got %.17g, expected %.17g\n", what, a, b, got, want);
    ++failures;
}

// one instance through both kernels' element loops; returns the source
static int step_instance(int choice, int policy, int K, int N, int nu, int nx, int fb, const std::vector<double> &sel, std::vector<double> &mem, int &age,
                         const double *tab, const double *x, const std::vector<double> &up, std::vector<double> &u, int &pick)
{
    int src = 0;
    for (int c = 0; c < nu; ++c) {                                // k_selected_inputs, element (b, c)
        const int s = sel_step_source(choice, fb, age, N);
        u[c] = sel_step_input(s, c, nu, nx, age, sel.data(), mem.data(), tab + (size_t)c * (nx + POL_TAIL), x, up[c]);
        if (c == 0) { src = s; pick = sel_step_pick(s, choice); }
    }
    for (int c = 0; c < N * nu; ++c)                              // k_selected_commit, element (b, c) of mem_u
        if (sel_step_remembered(src, policy, K, N)) mem[c] = sel[c];
    age = sel_step_next_age(src, policy, K, N, age);
    return src;
}

static void edges()
{
    const int N = 3, nu = 2, nx = 1;
    const double tab[2 * 6] = {1, 50, 60, 1, 0, 1, 1, 50, 60, 1, 0, 1};      // per channel [sel | on_at | off_at | u_on | u_off | mode]
    const double x[1] = {45.0};                                              // below on_at: the rule gives u_on = 1
    const int choices[3] = {-1, 0, 63}, policies[2] = {-1, 0}, ages[4] = {-1, 1, N - 1, N}, Ks[3] = {1, N - 1, N};
    int n = 0;
    for (int fb = 0; fb < 4; ++fb) for (int choice : choices) for (int policy : policies) for (int age0 : ages) for (int K : Ks) {
        if (choice < 0 && policy >= 0) continue;                  // refused by mld_set_selection, never made by a select call
        std::vector<double> sel((size_t)K * nu), mem((size_t)N * nu), up(nu, 0.0), u(nu, -9.0);
        for (int e = 0; e < K * nu; ++e) sel[e] = 100.0 + e;
        for (int e = 0; e < N * nu; ++e) mem[e] = -(1.0 + e);
        int age = age0, pick = -7;
        const int src = step_instance(choice, policy, K, N, nu, nx, fb, sel, mem, age, tab, x, up, u, pick);
        // the restatement
        const bool held = age0 >= 1 && age0 <= N - 1;
        const int want_src = choice >= 0 ? 3 : ((fb & MLD_FB_MEMORY) && held ? 1 : ((fb & MLD_FB_POLICY) ? 2 : -1));
        const bool kept = want_src == 3 && policy < 0 && K == N;
        const int want_age = kept ? 1 : (age0 >= 1 ? (age0 + 1 < N ? age0 + 1 : N) : age0);
        expect(src == want_src, "source", fb, choice, src, want_src);
        expect(pick == (want_src == 3 ? choice : -1), "pick", fb, choice, pick, want_src == 3 ? choice : -1);
        expect(age == want_age, "age", age0, K, age, want_age);
        for (int c = 0; c < nu; ++c) {
            const double want_u = want_src == 3 ? 100.0 + c : (want_src == 1 ? -(1.0 + age0 * nu + c) : (want_src == 2 ? 1.0 : 0.0));
            expect(u[c] == want_u, "u", want_src, c, u[c], want_u);
        }
        for (int e = 0; e < N * nu; ++e) { const double want_m = kept ? 100.0 + e : -(1.0 + e); expect(mem[e] == want_m, "mem_u", K, e, mem[e], want_m); }
        ++n;
    }
    expect(sel_kept_policy(-1, 2) == -1 && sel_kept_policy(0, 2) == -1 && sel_kept_policy(1, 2) == -1 && sel_kept_policy(2, 2) == 0 && sel_kept_policy(63, 2) == 61
           && sel_kept_policy(0, 0) == 0 && sel_kept_policy(63, 64) == -1, "kept policy", 0, 0, sel_kept_policy(63, 2), 61);
    printf("edges: %d combinations\n", n);
}

// Two steps, six instances, N_tilde = 3, one channel on one state; the thermostat on (1) at x <= 50, off (0) at x >= 60, in between what it was.  The
// selection of step s holds u[b, k] = 100 s + 10 b + k; the memory before step 0 holds -(10 b + k); ages -1, -1, 2, 3, 1, -1.
//   instance 0  choice 0 (a sequence)       1  choice 2, policy 0 (row 0 only)      2  no choice, age 2: the memory's row 2
//   instance 3  no choice, age 3: exhausted, the policy      4  choice 1 (a sequence), age 1      5  no choice, nothing remembered: the policy (x = 45: on)
static void example(int K)
{
    const int B = 6, N = 3, nu = 1, nx = 1, fb = MLD_FB_MEMORY | MLD_FB_POLICY;
    const double tab[6] = {1, 50, 60, 1, 0, 1};
    const int choice[2][6] = {{0, 2, -1, -1, 1, -1}, {-1, -1, -1, 0, 1, 2}}, policy[2][6] = {{-1, 0, -1, -1, -1, -1}, {-1, -1, -1, -1, -1, 0}};
    const double xs[2][6] = {{55, 55, 55, 55, 55, 45}, {55, 55, 55, 65, 55, 55}};
    const bool full = K == N;
    // K == N: instances 0 and 4 are remembered at step 0 (age 1), so at step 1 instance 0, without a choice, reads its row 1: 1.  K < N: nothing is
    // remembered, and instance 0 has nothing (age -1): the policy -- inside the band, u_prev = 0 is not u_on: off.
    const int want_src[2][6] = {{3, 3, 1, 2, 3, 2}, {full ? 1 : 2, 2, 2, 3, 3, 3}};
    const double want_u[2][6] = {{0, 12, -22, 0, 40, 1}, {full ? 1.0 : 0.0, 0, 0, 130, 140, 152}};
    const int want_pick[2][6] = {{0, 2, -1, -1, 1, -1}, {-1, -1, -1, 0, 1, 2}};
    const int want_age[2][2][6] = {{{-1, -1, 3, 3, 2, -1}, {-1, -1, 3, 3, 3, -1}}, {{1, -1, 3, 3, 1, -1}, {2, -1, 3, 1, 1, -1}}};
    std::vector<std::vector<double>> mem(B, std::vector<double>((size_t)N * nu));
    std::vector<int> age = {-1, -1, 2, 3, 1, -1};
    std::vector<std::vector<double>> up(B, std::vector<double>(nu, 0.0));
    for (int b = 0; b < B; ++b) for (int k = 0; k < N; ++k) mem[b][k] = -(10.0 * b + k);
    for (int s = 0; s < 2; ++s)
        for (int b = 0; b < B; ++b) {
            std::vector<double> sel((size_t)K * nu), u(nu);
            for (int k = 0; k < K; ++k) sel[k] = 100.0 * s + 10.0 * b + k;
            if (policy[s][b] >= 0) sel[0] = 100.0 * s + 10.0 * b + 2;      // a policy pick: row 0 is the rule's step 0 (here a made-up value), NaN behind it
            if (policy[s][b] >= 0) for (int k = 1; k < K; ++k) sel[k] = __builtin_nan("");
            int pick = -7;
            const int src = step_instance(choice[s][b], policy[s][b], K, N, nu, nx, fb, sel, mem[b], age[b], tab, &xs[s][b], up[b], u, pick);
            expect(src == want_src[s][b], "example source", s, b, src, want_src[s][b]);
            expect(u[0] == want_u[s][b], "example u", s, b, u[0], want_u[s][b]);
            expect(pick == want_pick[s][b], "example pick", s, b, pick, want_pick[s][b]);
            expect(age[b] == want_age[full][s][b], "example age", s, b, age[b], want_age[full][s][b]);
            if (src >= 0) up[b] = u;
        }
    // the memory at the end: K == N -- 0: step 0's sequence; 3: step 1's; 4: step 1's; the others as seeded.  K < N: all as seeded
    for (int b = 0; b < B; ++b) for (int k = 0; k < N; ++k) {
        double want = -(10.0 * b + k);
        if (full && b == 0) want = 10.0 * b + k;
        if (full && (b == 3 || b == 4)) want = 100.0 + 10.0 * b + k;
        expect(mem[b][k] == want, "example mem_u", b, k, mem[b][k], want);
    }
    printf("example K = %d: done\n", K);
}

int main()
{
    edges();
    example(3);
    example(2);
    printf(failures ? "%d FAILURES\n" : "selected_host_check: all values as written out\n", failures);
    return failures ? 1 : 0;
}
