// The per-instance core of k_rollout_risk (risk_instance, pyhybridcontrol_amd/csrc/rollout_risk.inc) on the CPU: with SM_HOST a "wave" is one lane and the LDS
// plain memory, so the keys, the bitonic network over the indexed arrays, the tree sums and the order statistics run under the host sanitizers.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/rollout_risk_host_check.cpp -o /tmp/rollout_risk_host_check && /tmp/rollout_risk_host_check
//
// Every buffer is exactly as long as the core may use (the sort region 64 + 64 doubles and 64 ints, every source S or S x ld entries, every output G or G x L,
// the rank table L x S), so the sanitizer sees an access past any of them.  What is expected: a naive restatement written out below -- an insertion sort by
// (value, c) with NaN last, a recursive tree sum, linear scans --, equal in every bit.  S = 1, 2, 3, 63, 64; every source; columns whose values all tie, with
// NaN and with both zeros; instances with n = 0 and n = 1; G = 1 and 64; L = 0 and 8.
#define SM_HOST
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mldgpu.h"
#include "rollout_risk.inc"

static int failures = 0;
static bool same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }
static void expect_d(const char *what, int S, int j, int l, double got, double want)
{
    if (same(got, want)) return;
    printf("FAIL %s (S = %d, column %d, level %d): got %.17g, expected %.17g\n", what, S, j, l, got, want);
    ++failures;
}
static void expect_i(const char *what, int S, int j, int l, int got, int want)
{
    if (got == want) return;
    printf("FAIL %s (S = %d, column %d, level %d): got %d, expected %d\n", what, S, j, l, got, want);
    ++failures;
}

// T, recursively: the sum of leaves [lo, lo + len) is the sum of its halves
static double tree(const double *leaf, int lo, int len)
{
    if (len == 1) return leaf[lo];
    volatile double a = tree(leaf, lo, len / 2), b = tree(leaf, lo + len / 2, len / 2);
    return a + b;
}

static unsigned rng_state = 12345u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

enum Fill { RANDOM, TIED, SPECIAL };

static void run(int S, int G, int L, int n_kpi, Fill fill, int ending_mode)
{
    const int ld = n_kpi | 1;      /* the staged stride; the padding is never read */
    std::vector<int> es(S), sw(S), nvio(S), kabove((size_t)S * ld), kchg((size_t)S * ld), src(G), q(G), idx((size_t)(L ? L * S : 1));
    std::vector<double> cost(S), mu(S), wv(S), ksum((size_t)S * ld), kmin((size_t)S * ld), kmax((size_t)S * ld), level(G), alpha(L);
    const double nanv = __builtin_nan(""), poison = 1e300;
    for (int c = 0; c < S; ++c) {
        /* endings: 0 all complete, 1 mixed, 2 none complete, 3 exactly one complete */
        es[c] = ending_mode == 0 ? 0 : ending_mode == 1 ? (int)(rnd() % 4) - 1 : ending_mode == 2 ? 1 + (c & 1) : (c == S / 2 ? 0 : -1);
        const bool ok = es[c] == 0;
        auto val = [&](int k) -> double {
            if (!ok) return nanv;                                 /* what the rollout writes for a trajectory that did not end 0 */
            if (fill == TIED) return 2.5;
            if (fill == SPECIAL) { const int r = (int)(rnd() % 6); return r == 0 ? nanv : r == 1 ? 0.0 : r == 2 ? -0.0 : r == 3 ? 1.0 : r == 4 ? -1.0 : 1.0; }
            return (double)((int)(rnd() % 41) - 20) / 8.0 + k;    /* dyadic, many ties */
        };
        cost[c] = val(0); mu[c] = val(1); wv[c] = val(2);
        sw[c] = ok ? (fill == TIED ? 3 : (int)(rnd() % 4)) : -1; nvio[c] = ok ? (fill == TIED ? 0 : (int)(rnd() % 3)) : -1;
        for (int k = 0; k < ld; ++k) {
            const size_t e = (size_t)c * ld + k;
            const bool padc = k >= n_kpi;
            ksum[e] = padc ? poison : val(3); kmin[e] = padc ? poison : val(4); kmax[e] = padc ? poison : val(5);
            kabove[e] = padc ? 999 : ok ? (fill == TIED ? 1 : (int)(rnd() % 5)) : -1; kchg[e] = padc ? 999 : ok ? (fill == TIED ? 2 : (int)(rnd() % 2)) : -1;
        }
    }
    for (int j = 0; j < G; ++j) { src[j] = j % RISK_N_SRC; q[j] = (j * 7) % n_kpi; level[j] = j % 5 == 4 ? (double)__builtin_inf() : (double)(j % 3) - 1.0; }
    const double alphas[8] = {1.0 / (double)S, 1.0, 1e-9, 0.5, 0.25, 0.75, 0.95, 0.05};
    for (int l = 0; l < L; ++l) { alpha[l] = alphas[l]; for (int n = 1; n <= S; ++n) idx[(size_t)l * S + n - 1] = risk_rank(alpha[l], n); }
    const size_t GL = (size_t)G * L;
    std::vector<double> mean(G, -7.0), mn(G, -7.0), mx(G, -7.0), qu(GL, -7.0), hi(GL, -7.0), lo(GL, -7.0);
    std::vector<int> mnc(G, -7), mxc(G, -7), ex(G, -7), quc(GL, -7), counts(4, -7);
    std::vector<double> sv(64), tt(64); std::vector<int> st(64);
    RiskIn I{};
    I.S = S; I.G = G; I.L = L; I.ld = ld; I.src = src.data(); I.q = q.data(); I.level = level.data(); I.idx = idx.data();
    I.es = es.data(); I.cost = cost.data(); I.mu = mu.data(); I.wv = wv.data(); I.sw = sw.data(); I.nvio = nvio.data();
    I.ksum = ksum.data(); I.kmin = kmin.data(); I.kmax = kmax.data(); I.kabove = kabove.data(); I.kchg = kchg.data();
    RiskOut O{};
    O.mean = mean.data(); O.min = mn.data(); O.max = mx.data(); O.min_c = mnc.data(); O.max_c = mxc.data(); O.n_exceed = ex.data();
    O.quantile = L ? qu.data() : nullptr; O.cvar_hi = L ? hi.data() : nullptr; O.cvar_lo = L ? lo.data() : nullptr; O.quantile_c = L ? quc.data() : nullptr;
    O.counts = counts.data();
    risk_instance(I, O, sv.data(), tt.data(), st.data(), 0);

    /* the naive restatement */
    int cnt[4] = {0, 0, 0, 0};
    for (int c = 0; c < S; ++c) cnt[es[c] == 0 ? 0 : es[c] == 1 ? 1 : es[c] == 2 ? 2 : 3] += 1;
    for (int k = 0; k < 4; ++k) expect_i("counts", S, -1, k, counts[k], cnt[k]);
    const int n = cnt[0];
    for (int j = 0; j < G; ++j) {
        std::vector<double> g(S);
        for (int c = 0; c < S; ++c) {
            const size_t e = (size_t)c * ld + q[j];
            switch (src[j]) {
            case 0: g[c] = cost[c]; break; case 1: g[c] = mu[c]; break; case 2: g[c] = wv[c]; break; case 3: g[c] = sw[c]; break; case 4: g[c] = nvio[c]; break;
            case 5: g[c] = ksum[e]; break; case 6: g[c] = kmin[e]; break; case 7: g[c] = kmax[e]; break; case 8: g[c] = kabove[e]; break; default: g[c] = kchg[e];
            }
        }
        double leaf[64];
        for (int c = 0; c < 64; ++c) leaf[c] = c < S && es[c] == 0 ? g[c] : 0.0;
        expect_d("mean", S, j, -1, mean[j], n ? tree(leaf, 0, 64) / (double)n : nanv);
        /* insertion sort of the complete c by (value, c), NaN last: c ascending is inserted behind every element that is not greater */
        std::vector<int> ord;
        for (int c = 0; c < S; ++c) {
            if (es[c] != 0) continue;
            size_t at = ord.size();
            while (at > 0 && !(g[c] != g[c]) && (g[ord[at - 1]] != g[ord[at - 1]] || g[c] < g[ord[at - 1]])) --at;
            ord.insert(ord.begin() + at, c);
        }
        double lo_v = (double)__builtin_inf(), hi_v = -(double)__builtin_inf(); int lo_c = -1, hi_c = -1, above = 0;
        for (int c = 0; c < S; ++c) {
            if (es[c] != 0) continue;
            if (g[c] < lo_v) { lo_v = g[c]; lo_c = c; }
            if (g[c] > hi_v) { hi_v = g[c]; hi_c = c; }
            above += g[c] > level[j];
        }
        expect_d("min", S, j, -1, mn[j], lo_v); expect_i("min_c", S, j, -1, mnc[j], lo_c);
        expect_d("max", S, j, -1, mx[j], hi_v); expect_i("max_c", S, j, -1, mxc[j], hi_c);
        expect_i("n_exceed", S, j, -1, ex[j], above);
        for (int l = 0; l < L; ++l) {
            const size_t o = (size_t)j * L + l;
            if (n == 0) {
                expect_d("quantile", S, j, l, qu[o], nanv); expect_i("quantile_c", S, j, l, quc[o], -1);
                expect_d("cvar_hi", S, j, l, hi[o], nanv); expect_d("cvar_lo", S, j, l, lo[o], nanv);
                continue;
            }
            int i = 0;
            while (!((double)(i + 1) >= alpha[l] * (double)n)) ++i;
            double a[64], b[64];
            for (int r = 0; r < 64; ++r) { a[r] = r >= i && r < n ? g[ord[r]] : 0.0; b[r] = r <= i ? g[ord[r]] : 0.0; }
            expect_d("quantile", S, j, l, qu[o], g[ord[i]]); expect_i("quantile_c", S, j, l, quc[o], ord[i]);
            expect_d("cvar_hi", S, j, l, hi[o], tree(a, 0, 64) / (double)(n - i)); expect_d("cvar_lo", S, j, l, lo[o], tree(b, 0, 64) / (double)(i + 1));
        }
    }
}

int main()
{
    /* the rank table's corners */
    if (risk_rank(1.0, 64) != 63 || risk_rank(1e-9, 64) != 0 || risk_rank(1.0 / 3.0, 3) != 0 || risk_rank(0.5, 4) != 1 || risk_rank(0.5, 5) != 2 || risk_rank(1.0, 1) != 0) {
        printf("FAIL risk_rank\n"); ++failures;
    }
    const int sizes[5] = {1, 2, 3, 63, 64};
    int runs = 0;
    for (int s = 0; s < 5; ++s)
        for (int fill = 0; fill < 3; ++fill)
            for (int ending = 0; ending < 4; ++ending) {
                run(sizes[s], 64, 8, 64, (Fill)fill, ending); ++runs;      /* G = 64 over all ten sources, n_kpi = 64 */
                run(sizes[s], 1, 0, 1, (Fill)fill, ending); ++runs;        /* one column, no level */
                run(sizes[s], 13, 3, 5, (Fill)fill, ending); ++runs;
            }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("rollout risk host check: %d instances, every figure as the naive restatement gives it\n", runs);
    return 0;
}
