// The byte rule of a MIP start taken from a rollout (ws_source, ws_element, pyhybridcontrol_amd/csrc/warm_rollout.inc) on the CPU: the per-element body of
// k_warm_from_rollout is a host-compilable function, so the loop the kernel runs per (instance, binary) runs here under the host sanitizers, every array
// sized to the byte -- the first and the last binary, the last step's last column, the last instance, and a 255 first byte under keep.  Every value below
// is worked out by hand.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/start_rollout_host_check.cpp -o /tmp/start_rollout_host_check && /tmp/start_rollout_host_check
//
// Five instances, N_tilde = 3, nv = 4, the binaries are columns 1 and 3 of every step (n_bin = 6; the last one is the last double of a row of v).
// v[b, step, pos] = ((b + step + pos) % 2 ? 0.75 : 0.25), except v[0, 2, 3] = NaN (rounds to 0) and v[0, 0, 1] = 0.5 (not above one half: 0).
// Endings: complete, infeasible, complete, declined, not attempted.
#include <math.h>
#include <stdio.h>
#include <vector>

#include "warm_rollout.inc"

static int failures = 0;
static void expect(bool ok, const char *what, int b, int k, int got, int want)
{
    if (ok) return;
    printf("FAIL %s[instance %d, binary %d]: got %d, expected %d\n", what, b, k, got, want);
    ++failures;
}

static void run(const char *name, const std::vector<unsigned char> *old, const int want_src[5], const unsigned char want[5][6])
{
    const int B = 5, N = 3, nv = 4, nb = 6;
    const std::vector<int> bins = {1, 3, 5, 7, 9, 11};
    const std::vector<int> end = {0, 1, 0, 2, -1};
    std::vector<double> v((size_t)B * N * nv);
    for (int b = 0; b < B; ++b) for (int s = 0; s < N; ++s) for (int c = 0; c < nv; ++c) v[((size_t)b * N + s) * nv + c] = (b + s + c) % 2 ? 0.75 : 0.25;
    v[(0 * N + 2) * nv + 3] = nan("");
    v[(0 * N + 0) * nv + 1] = 0.5;
    std::vector<unsigned char> warm = old ? *old : std::vector<unsigned char>((size_t)B * nb, 77);
    std::vector<int> src(B, 99);
    for (unsigned long long t = 0; t < (unsigned long long)B * nb; ++t) {      // k_warm_from_rollout, thread t
        const int s = ws_element(t, nb, nv, bins.data(), v.data(), (size_t)N * nv, end.data(), old ? old->data() : nullptr, warm.data());
        if (t % nb == 0) src[t / nb] = s;
    }
    for (int b = 0; b < B; ++b) {
        expect(src[b] == want_src[b], "source", b, 0, src[b], want_src[b]);
        for (int k = 0; k < nb; ++k) expect(warm[(size_t)b * nb + k] == want[b][k], "start", b, k, warm[(size_t)b * nb + k], want[b][k]);
    }
    printf("%s: done\n", name);
}

int main()
{
    // instance 0: (0+s+c) odd -> 1: binaries (s, c) = (0,1) 0.5 -> 0, (0,3) 1, (1,1) 0, (1,3) 0, (2,1) 1, (2,3) NaN -> 0
    // instance 2: the same parities without the exceptions: 1, 1, 0, 0, 1, 1
    const unsigned char fresh[5][6] = {{0, 1, 0, 0, 1, 0}, {255, 255, 255, 255, 255, 255}, {1, 1, 0, 0, 1, 1}, {255, 255, 255, 255, 255, 255}, {255, 255, 255, 255, 255, 255}};
    const int src_fresh[5] = {1, -1, 1, -2, -3};
    run("every row written", nullptr, src_fresh, fresh);
    // keep: rows 0, 1 and 4 have a start (first byte 0 / 1), rows 2 and 3 have none (first byte 255, the rest whatever was there)
    const std::vector<unsigned char> old = {1, 0, 1, 0, 1, 0,  0, 0, 0, 0, 0, 0,  255, 9, 9, 9, 9, 9,  255, 255, 255, 255, 255, 255,  1, 1, 1, 1, 1, 1};
    const unsigned char kept[5][6] = {{1, 0, 1, 0, 1, 0}, {0, 0, 0, 0, 0, 0}, {1, 1, 0, 0, 1, 1}, {255, 255, 255, 255, 255, 255}, {1, 1, 1, 1, 1, 1}};
    const int src_kept[5] = {0, 0, 1, -2, 0};
    run("keep", &old, src_kept, kept);
    // the source rule on its own
    expect(ws_source(0, true, 255) == 1 && ws_source(0, true, 0) == 0 && ws_source(0, false, 0) == 1, "ws_source keep", 0, 0, ws_source(0, true, 255), 1);
    expect(ws_source(1, false, 0) == -1 && ws_source(2, true, 255) == -2 && ws_source(-1, false, 1) == -3 && ws_source(1, true, 1) == 0, "ws_source endings", 0, 0, ws_source(1, false, 0), -1);
    printf(failures ? "%d FAILURES\n" : "start_rollout_host_check: all values as written out\n", failures);
    return failures ? 1 : 0;
}
