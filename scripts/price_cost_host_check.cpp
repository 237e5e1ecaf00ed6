// The two formulas of resident price profiles (price_window_sum, price_cost_elem, stage_cost_value, pyhybridcontrol_amd/csrc/prices.inc) and the window
// rule's bounds test (profile_start_ok, profiles.inc) on the CPU: the functions the kernels k_price_cost and k_stage_cost call per element are
// host-compilable, so the loops the kernels run per (instance, element) run here under the host sanitizers, every array sized to the byte.
//
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/price_cost_host_check.cpp -o /tmp/price_cost_host_check && /tmp/price_cost_host_check
//
// Checked: a start at every boundary of the window rule (0, the largest valid value, one beyond it, -1, values near INT64_MAX, steps near INT_MAX), with a
// read of the window's first and last element out of an exactly sized library wherever the rule says "valid"; and both formulas against a long-double
// evaluation of the same sums, within the classical bound of recursive summation (terms x 2^-53 relative to the sum of the absolute terms).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <cmath>
#include <vector>

#include "profiles.inc"
#include "prices.inc"

static int failures = 0;
static void expect(bool ok, const char *what, long long a, long long b)
{
    if (ok) return;
    printf("FAIL %s (%lld, %lld)\n", what, a, b);
    ++failures;
}

static double urand(unsigned &s) { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24); }

static void window_rule()
{
    const int n_chan = 3, N = 5;
    const long long rows = 11, lib_len = rows * n_chan;
    std::vector<double> lib((size_t)lib_len);
    for (long long i = 0; i < lib_len; ++i) lib[(size_t)i] = (double)i;
    for (int len : {N, 1})
        for (int step : {0, 2}) {
            const long long last = lib_len - ((long long)step + len) * n_chan;      // the largest valid start
            const long long cand[] = {0, 1, last - 1, last, last + 1, -1, -n_chan, lib_len, INT64_MAX, INT64_MAX - 1, INT64_MIN, INT64_MAX - (long long)(step + len) * n_chan};
            for (long long s : cand) {
                const bool ok = profile_start_ok(s, lib_len, step, len, n_chan), want = s >= 0 && s <= last;
                expect(ok == want, "profile_start_ok", s, step);
                if (!ok) continue;
                const double *win = lib.data() + s + (long long)step * n_chan;      // what k_price_cost stages and k_stage_cost reads
                double sum = 0.0;
                for (int i = 0; i < len * n_chan; ++i) sum += win[i];               // (ASan: an exactly sized library)
                expect(win[len * n_chan - 1] == (double)(s + ((long long)step + len) * n_chan - 1), "the window's last element", s, step);
                (void)sum;
            }
        }
    // steps and widths at the edge of int: the test itself must not overflow
    expect(!profile_start_ok(0, lib_len, INT_MAX - 1, 1, INT_MAX), "huge step and width", 0, 0);
    expect(!profile_start_ok(INT64_MAX, INT64_MAX, INT_MAX - N, N, 1), "start at INT64_MAX", 0, 0);
    expect(profile_start_ok(INT64_MAX - 7, INT64_MAX, 2, N, 1), "a library of INT64_MAX doubles, the last window", 0, 0);
    expect(!profile_start_ok(INT64_MAX - 6, INT64_MAX, 2, N, 1), "a library of INT64_MAX doubles, one beyond", 0, 0);
    expect(!profile_start_ok(0, 0, 0, 1, 1) && !profile_start_ok(0, 2, 0, 1, 3), "a library shorter than one element run", 0, 0);
}

static void formulas()
{
    unsigned seed = 12345u;
    const double u = std::ldexp(1.0, -53);
    for (int n_chan : {1, 3})
        for (int N : {1, 5, 25}) {
            const int nv = 7, ny = 2, W = nv;
            std::vector<double> win((size_t)N * n_chan), a((size_t)n_chan * W), s((size_t)n_chan * W), S((size_t)n_chan);
            for (double &t : win) t = 0.5 + urand(seed);
            for (double &t : a) t = urand(seed) - 0.5;
            for (double &t : s) t = urand(seed) - 0.5;
            for (int c = 0; c < n_chan; ++c) {
                S[(size_t)c] = price_window_sum(win.data(), N, n_chan, c);
                long double ref = 0.0L, mag = 0.0L;
                for (int k = 0; k < N; ++k) { ref += win[(size_t)k * n_chan + c]; mag += std::fabs(win[(size_t)k * n_chan + c]); }
                expect(std::fabs((double)((long double)S[(size_t)c] - ref)) <= (double)(N * u * mag), "price_window_sum", N, c);
            }
            for (int k = 0; k < N; ++k)
                for (int j = 0; j < W; ++j) {
                    const double *pk = win.data() + (size_t)k * n_chan;
                    const double got = price_cost_elem(a.data(), s.data(), pk, S.data(), n_chan, W, j), got_y = price_cost_elem(a.data(), nullptr, pk, S.data(), n_chan, W, j);
                    long double ref = 0.0L, ref_y = 0.0L, mag = 0.0L;
                    for (int c = 0; c < n_chan; ++c) {
                        ref_y += (long double)a[(size_t)c * W + j] * pk[c];
                        ref += (long double)a[(size_t)c * W + j] * pk[c] + (long double)s[(size_t)c * W + j] * S[(size_t)c];
                        mag += std::fabs((long double)a[(size_t)c * W + j] * pk[c]) + std::fabs((long double)s[(size_t)c * W + j] * S[(size_t)c]);
                    }
                    expect(std::fabs((double)((long double)got - ref)) <= (double)((2 * n_chan + 2) * u * mag), "price_cost_elem", k, j);
                    expect(std::fabs((double)((long double)got_y - ref_y)) <= (double)((n_chan + 1) * u * mag), "price_cost_elem without the sum term", k, j);
                }
            // the stage cost of one record
            std::vector<double> wv((size_t)n_chan * nv), wy((size_t)n_chan * ny), v((size_t)nv), y((size_t)ny);
            for (double &t : wv) t = urand(seed) - 0.5;
            for (double &t : wy) t = urand(seed) - 0.5;
            for (double &t : v) t = 4.0 * urand(seed) - 2.0;
            for (double &t : y) t = 4.0 * urand(seed) - 2.0;
            const double got = stage_cost_value(wv.data(), wy.data(), win.data(), v.data(), y.data(), n_chan, nv, ny);
            long double ref = 0.0L, mag = 0.0L;
            for (int c = 0; c < n_chan; ++c) {
                long double in = 0.0L, im = 0.0L;
                for (int j = 0; j < nv; ++j) { in += (long double)wv[(size_t)c * nv + j] * v[(size_t)j]; im += std::fabs((long double)wv[(size_t)c * nv + j] * v[(size_t)j]); }
                for (int j = 0; j < ny; ++j) { in += (long double)wy[(size_t)c * ny + j] * y[(size_t)j]; im += std::fabs((long double)wy[(size_t)c * ny + j] * y[(size_t)j]); }
                ref += (long double)win[(size_t)c] * in; mag += std::fabs((long double)win[(size_t)c]) * im;
            }
            expect(std::fabs((double)((long double)got - ref)) <= (double)((nv + ny + n_chan + 3) * u * mag), "stage_cost_value", n_chan, N);
            // z times price: one weight of 1, everything else 0 -- exact
            std::fill(wv.begin(), wv.end(), 0.0); std::fill(wy.begin(), wy.end(), 0.0);
            wv[3] = 1.0;
            expect(stage_cost_value(wv.data(), wy.data(), win.data(), v.data(), y.data(), n_chan, nv, ny) == win[0] * v[3], "z times price", n_chan, N);
        }
}

int main()
{
    window_rule();
    formulas();
    printf(failures ? "%d FAILURES\n" : "price_cost_host_check: the window rule and both formulas as stated\n", failures);
    return failures ? 1 : 0;
}
