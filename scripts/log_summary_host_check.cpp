// The rule of the campaign KPIs (ls_dot, ls_add_term, ls_priced, ls_functional, ls_accumulate, ls_fixed_accumulate, ls_index;
// pyhybridcontrol_amd/csrc/log_summary.inc) on the CPU: the functions k_log_summary calls per record are host-compilable, so the loops the kernel runs per
// (instance, KPI) run here under the host sanitizers, every array sized to the byte.
//
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/log_summary_host_check.cpp -o /tmp/log_summary_host_check && /tmp/log_summary_host_check
//
// Checked: the functional with every subset of the five tables against the sums written out by hand in the stated order (equal bits) and against a
// long-double evaluation within the bound of recursive summation; the accumulate rule with ties, NaN values, an all-skipped range and count == 0; the
// per-instance block; and the 64-bit record index at cap x batch x width just past 2^31 and 2^32 -- computed, not allocated.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <cmath>
#include <limits>
#include <vector>

#include "log_summary.inc"

static int failures = 0;
static void expect(bool ok, const char *what, long long a, long long b)
{
    if (ok) return;
    printf("FAIL %s (%lld, %lld)\n", what, a, b);
    ++failures;
}

static double urand(unsigned &s) { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24); }
static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }

static void functional()
{
    unsigned seed = 2024u;
    const int width[5] = {3, 11, 1, 4, 3};
    const double u = std::ldexp(1.0, -53);
    std::vector<double> w[5], f[5];
    for (int t = 0; t < 5; ++t) {
        w[t].resize((size_t)width[t]); f[t].resize((size_t)width[t]);      // exactly sized: a read past a table's end is ASan's
        for (double &v : w[t]) v = urand(seed) - 0.5;
        for (double &v : f[t]) v = 40.0 * urand(seed) - 20.0;
    }
    for (int mask = 1; mask < 32; ++mask) {
        const double *wp[5], *fp[5];
        for (int t = 0; t < 5; ++t) { wp[t] = (mask >> t & 1) ? w[t].data() : nullptr; fp[t] = f[t].data(); }
        const double got = ls_functional(wp, 1, fp, width);
        // by hand, in the stated order
        double want = 0.0; bool first = true; long double ref = 0.0L, mag = 0.0L; int terms = 0;
        for (int t = 0; t < 5; ++t) {
            if (!(mask >> t & 1)) continue;
            volatile double s = 0.0;
            for (int i = 0; i < width[t]; ++i) { volatile double p = w[t][(size_t)i] * f[t][(size_t)i]; s = s + p; ref += (long double)w[t][(size_t)i] * f[t][(size_t)i]; mag += std::fabs((long double)p); ++terms; }
            if (first) want = s; else { volatile double a = want + s; want = a; }
            first = false;
        }
        expect(same_bits(got, want), "ls_functional against the sums by hand", mask, 0);
        expect(std::fabs((double)((long double)got - ref)) <= (double)((terms + 5) * u * mag), "ls_functional against long double", mask, 0);
    }
    // a strided table (the device's KPI-minor layout) gives the bits of the contiguous one
    const int Q = 7, n = width[1];
    std::vector<double> wt((size_t)n * Q, 0.0);
    for (int i = 0; i < n; ++i) wt[(size_t)i * Q + 3] = w[1][(size_t)i];
    expect(same_bits(ls_dot(wt.data() + 3, (size_t)Q, f[1].data(), n), ls_dot(w[1].data(), 1, f[1].data(), n)), "ls_dot with a stride", 0, 0);
    // a selector is exact; a table that is not given adds no term: a NaN field behind it does not reach f
    std::vector<double> sel((size_t)width[1], 0.0); sel[5] = 1.0;
    std::vector<double> nanf((size_t)width[0], std::numeric_limits<double>::quiet_NaN());
    const double *wp[5] = {nullptr, sel.data(), nullptr, nullptr, nullptr}, *fp[5] = {nanf.data(), f[1].data(), f[2].data(), f[3].data(), f[4].data()};
    expect(ls_functional(wp, 1, fp, width) == f[1][5], "a unit selector", 0, 0);
    expect(ls_priced(1.5, 2.0) == 3.0, "ls_priced", 0, 0);
}

static void accumulate()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    LsAcc a; ls_acc_init(a);
    // count == 0 / an all-skipped range: nothing is accumulated
    expect(a.sum == 0.0 && a.min == inf && a.max == -inf && a.min_step == -1 && a.max_step == -1 && a.n_above == 0 && a.n_changes == 0, "the empty values", 0, 0);
    // values with ties at records 12 / 15 (max) and 11 / 14 (min), a NaN at 13; records 10 .. 16 are stepped
    const double f[7] = {1.0, -2.0, 5.0, nan, -2.0, 5.0, 5.0};
    for (int k = 0; k < 7; ++k) ls_accumulate(a, f[k], 0.5, 10 + k);
    expect(a.min == -2.0 && a.min_step == 11, "the first attaining record wins the minimum", a.min_step, 0);
    expect(a.max == 5.0 && a.max_step == 12, "the first attaining record wins the maximum", a.max_step, 0);
    expect(a.n_above == 4, "n_above: a NaN is not above", a.n_above, 0);
    expect(a.n_changes == 5, "n_changes: 1 -> -2 -> 5 -> NaN -> -2 -> 5 = 5, the last 5 -> 5 none", a.n_changes, 0);
    expect(a.sum != a.sum, "a NaN reaches the sum", 0, 0);
    // the sum's order: ((0 + a) + b) + c
    LsAcc s; ls_acc_init(s);
    const double v[3] = {1.0, std::ldexp(1.0, -53), std::ldexp(1.0, -53)};
    for (int k = 0; k < 3; ++k) ls_accumulate(s, v[k], inf, k);
    expect(s.sum == 1.0, "the sum is serial: 1 + 2^-53 + 2^-53 rounds to 1 twice", 0, 0);
    expect(s.n_above == 0 && s.n_changes == 1, "thresh = +inf; one change", s.n_above, s.n_changes);
    // the per-instance block
    LsFixed x; ls_fixed_init(x, true);
    expect(x.vio_max == -inf && x.vio_step == -1 && x.n_stepped == 0 && x.n_vio == 0 && x.nodes_total == 0 && x.n_source[0] == 0, "the empty block", 0, 0);
    const double vio[5] = {-1.0, 3e-6, nan, 3e-6, 1e-7};
    const bool stepped[5] = {true, true, false, true, true};
    const int src[5] = {0, 1, -1, 1, 2};
    for (int k = 0; k < 5; ++k) ls_fixed_accumulate(x, stepped[k], vio[k], 2000000000, src[k], true, 1e-6, 4 + k);
    expect(x.n_stepped == 4 && x.vio_max == 3e-6 && x.vio_step == 5 && x.n_vio == 2, "vio: the first of the ties, the skipped record not counted", x.vio_step, x.n_vio);
    expect(x.nodes_total == 10000000000LL, "nodes_total is 64-bit and counts every record", x.nodes_total, 0);
    expect(x.n_source[0] == 1 && x.n_source[1] == 2 && x.n_source[2] == 1, "n_source", x.n_source[1], 0);
    LsFixed y; ls_fixed_init(y, false);
    ls_fixed_accumulate(y, true, 0.0, 1, 7, false, 1e-6, 0);
    expect(y.n_source[0] == -1 && y.n_source[1] == -1 && y.n_source[2] == -1, "no source array: -1", 0, 0);
    expect(ls_stepped(0.0) && ls_stepped(inf) && !ls_stepped(nan), "the stepped rule", 0, 0);
}

static void index64()
{
    // cfg4 shard: batch 32 768, nv = 23: record 2 850 of v starts past 2^31 elements, record 5 699 past 2^32
    const long long batch = 32768, width = 23;
    const long long two31 = 1LL << 31, two32 = 1LL << 32;
    const long long k31 = two31 / (batch * width) + 1, k32 = two32 / (batch * width) + 1;
    const size_t i31 = ls_index(k31, batch, batch - 1, width, width - 1), i32 = ls_index(k32, batch, batch - 1, width, width - 1);
    expect(i31 == (size_t)((k31 * batch + batch - 1) * width + width - 1) && i31 > (size_t)two31, "the index just past 2^31", (long long)i31, k31);
    expect(i32 == (size_t)((k32 * batch + batch - 1) * width + width - 1) && i32 > (size_t)two32, "the index just past 2^32", (long long)i32, k32);
    expect((long long)(int)i31 != (long long)i31, "a 32-bit index would have wrapped", 0, 0);
    expect(ls_index(0, batch, 0, width, 0) == 0 && ls_index(1, batch, 0, width, 0) == (size_t)(batch * width), "the first records", 0, 0);
}

int main()
{
    functional();
    accumulate();
    index64();
    printf(failures ? "%d FAILURES\n" : "log_summary_host_check: the functional, the accumulate rule and the record index as stated\n", failures);
    return failures ? 1 : 0;
}
