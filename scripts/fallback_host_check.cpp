// The choice of the source of u and the ageing of the plan memory (fb_source, fb_input, fb_next_age, pyhybridcontrol_amd/csrc/fallback.inc) on the CPU: the
// per-element bodies of k_fallback_inputs and k_fallback_commit are host-compilable functions (SM_HOST, as small_lds.inc), so the loops the kernels run per
// (instance, channel) and per memory element run here under the host sanitizers, every array sized to the byte.  The example is the one of
// tests/test_fallback_host.py, every value below worked out by hand.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/fallback_host_check.cpp -o /tmp/fallback_host_check && /tmp/fallback_host_check
//
// Three steps, four instances, N_tilde = 3, one channel on one state; the thermostat on (1) at x <= 50, off (0) at x >= 60, in between what it was.  The plan
// of step s holds u[b, k] = 100 s + 10 b + k; the memory before step 0 holds -(10 b + k), and only instance 2 remembers anything: age 2.
#define SM_HOST
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "mldgpu.h"
#include "rollout.inc"
#include "fallback.inc"

static int failures = 0;
static void expect(bool ok, const char *what, int s, int b, double got, double want)
{
    if (ok) return;
    printf("FAIL %s[step %d, instance %d]: got %.17g, expected %.17g\n", what, s, b, got, want);
    ++failures;
}

struct Want { int src[3][4]; double u[3][4]; int age[3][4]; };

static void run(const char *name, int fb, const Want &w)
{
    const int B = 4, N = 3, nu = 1, nx = 1, nv = 2;               // nv = 2: the plan's row holds [u; one auxiliary] per step, as the commit's gather strides
    const double tab[6] = {1, 50, 60, 1, 0, 1};                   // [sel | on_at | off_at | u_on | u_off | mode]
    const bool usable[3][4] = {{true, true, false, false}, {true, false, false, false}, {true, false, false, false}};
    const double xs[3][4] = {{55, 55, 55, 45}, {55, 55, 55, 55}, {55, 55, 65, 65}};
    std::vector<std::vector<double>> mem(B, std::vector<double>((size_t)N * nu));      // one allocation per instance: a read past a row is seen
    std::vector<int> age = {-1, -1, 2, -1};
    std::vector<double> up(B, 0.0);
    for (int b = 0; b < B; ++b) for (int k = 0; k < N; ++k) mem[b][k] = -(10.0 * b + k);
    for (int s = 0; s < 3; ++s) {
        std::vector<std::vector<double>> plan(B, std::vector<double>((size_t)N * nv, -7.0));
        for (int b = 0; b < B; ++b) for (int k = 0; k < N; ++k) plan[b][k * nv] = 100.0 * s + 10.0 * b + k;
        std::vector<int> src(B);
        std::vector<double> u((size_t)B * nu);
        for (int b = 0; b < B; ++b)                               // k_fallback_inputs, element (b, c)
            for (int c = 0; c < nu; ++c) {
                const int sc = fb_source(usable[s][b], fb, age[b], N);
                u[b * nu + c] = fb_input(sc, c, nu, nx, age[b], plan[b].data(), mem[b].data(), tab + (size_t)c * (nx + POL_TAIL), &xs[s][b], up[b * nu + c]);
                if (c == 0) src[b] = sc;
            }
        for (int b = 0; b < B; ++b) {                             // k_fallback_commit, element (b, c) of mem_u
            for (int c = 0; c < N * nu; ++c)
                if (src[b] == FB_PLAN) { const int k = c / nu, j = c - k * nu; mem[b][c] = plan[b][k * nv + j]; }
            age[b] = fb_next_age(src[b], age[b], N);
        }
        for (int b = 0; b < B; ++b) {
            expect(src[b] == w.src[s][b], "source", s, b, src[b], w.src[s][b]);
            expect(u[b] == w.u[s][b], "u", s, b, u[b], w.u[s][b]);
            expect(age[b] == w.age[s][b], "age", s, b, age[b], w.age[s][b]);
            if (src[b] >= 0) up[b] = u[b];                        // every attempted instance advances here
        }
    }
    const double want_mem[4][3] = {{200, 201, 202}, {10, 11, 12}, {-20, -21, -22}, {-30, -31, -32}};
    for (int b = 0; b < B; ++b) for (int k = 0; k < N; ++k) expect(mem[b][k] == want_mem[b][k], "mem_u", k, b, mem[b][k], want_mem[b][k]);
    printf("%s: done\n", name);
}

int main()
{
    const int ages[3][4] = {{1, 1, 3, -1}, {1, 2, 3, -1}, {1, 3, 3, -1}};      // 3 = N_tilde is the cap; -1 stays -1 whatever is applied
    Want both = {{{0, 0, 1, 2}, {0, 1, 2, 2}, {0, 1, 2, 2}}, {{0, 10, -22, 1}, {100, 11, 0, 1}, {200, 12, 0, 0}}, {}};
    Want memory = {{{0, 0, 1, -1}, {0, 1, -1, -1}, {0, 1, -1, -1}}, {{0, 10, -22, 0}, {100, 11, 0, 0}, {200, 12, 0, 0}}, {}};
    Want rule = {{{0, 0, 2, 2}, {0, 2, 2, 2}, {0, 2, 2, 2}}, {{0, 10, 0, 1}, {100, 0, 0, 1}, {200, 0, 0, 0}}, {}};
    Want none = {{{0, 0, -1, -1}, {0, -1, -1, -1}, {0, -1, -1, -1}}, {{0, 10, 0, 0}, {100, 0, 0, 0}, {200, 0, 0, 0}}, {}};
    for (Want *w : {&both, &memory, &rule, &none}) for (int s = 0; s < 3; ++s) for (int b = 0; b < 4; ++b) w->age[s][b] = ages[s][b];
    run("memory and policy", MLD_FB_MEMORY | MLD_FB_POLICY, both);
    run("memory only", MLD_FB_MEMORY, memory);
    run("policy only", MLD_FB_POLICY, rule);
    run("no source allowed", 0, none);
    // the edges of the ageing on their own
    expect(fb_next_age(FB_PLAN, -1, 3) == 1 && fb_next_age(FB_PLAN, 3, 3) == 1, "a plan is remembered", 0, 0, fb_next_age(FB_PLAN, -1, 3), 1);
    expect(fb_next_age(FB_NONE, 2, 3) == 3 && fb_next_age(FB_POLICY, 3, 3) == 3 && fb_next_age(FB_MEMORY, 1, 3) == 2, "ageing", 0, 0, fb_next_age(FB_NONE, 2, 3), 3);
    expect(fb_next_age(FB_NONE, -1, 3) == -1 && fb_next_age(FB_POLICY, -1, 3) == -1, "nothing remembered stays", 0, 0, fb_next_age(FB_NONE, -1, 3), -1);
    expect(fb_source(false, MLD_FB_MEMORY, 1, 1) == FB_NONE && fb_source(false, MLD_FB_MEMORY, 1, 2) == FB_MEMORY, "N_tilde = 1 has no usable row", 0, 0, fb_source(false, MLD_FB_MEMORY, 1, 1), FB_NONE);
    printf(failures ? "%d FAILURES\n" : "fallback_host_check: all values as written out\n", failures);
    return failures ? 1 : 0;
}
