// The selection rule of k_plan_select (pyhybridcontrol_amd/csrc/plan_select.inc) on the CPU: the statistic of a candidate, its admissibility, THE ORDER, the
// serial scan and a simulated wave butterfly of the same comparator run under the host sanitizers.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipyhybridcontrol_amd/csrc scripts/plan_select_host_check.cpp -o /tmp/plan_select_host_check && /tmp/plan_select_host_check
//
// Every risk array is exactly as long as the rule may read (G or G x L entries per candidate, counts 4), so the sanitizer sees an access past any of them.
// What is expected: a naive restatement written out below -- the value by a chain of ifs, the admissibility by a loop, the choice by a linear scan that keeps
// the first least value.  P = 1 .. 64; random dyadic values with many ties, all-tied values, NaN, both infinities and both zeros; every kind as objective;
// 0, 1 and 8 constraints; min_complete 1 and S; nobody admissible (min_complete beyond S).  The butterfly is the device's: 64 lanes, lane p >= P without a candidate, six xor steps.
#define SM_HOST
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mldgpu.h"
#include "plan_select.inc"

static int failures = 0;
static bool same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }
static void fail(const char *what, int P, int b, double got, double want)
{
    printf("FAIL %s (P = %d, instance %d): got %.17g, expected %.17g\n", what, P, b, got, want);
    ++failures;
}

static unsigned rng_state = 2463534242u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

enum Fill { RANDOM, TIED, SPECIAL };

static double draw(Fill fill)
{
    const double nanv = __builtin_nan(""), inf = (double)__builtin_inf();
    if (fill == TIED) return 2.5;
    if (fill == SPECIAL) { const int r = (int)(rnd() % 8); return r == 0 ? nanv : r == 1 ? 0.0 : r == 2 ? -0.0 : r == 3 ? inf : r == 4 ? -inf : r == 5 ? 1.0 : -1.0; }
    return (double)((int)(rnd() % 9) - 4) / 4.0;      /* dyadic, many ties */
}

// the device's butterfly over 64 lanes, with the rule's comparator
static int butterfly(const double *v, const unsigned char *ok, int P, double &score, int &n_adm)
{
    double lv[64]; int lp[64], ln[64];
    for (int l = 0; l < 64; ++l) { const bool has = l < P && ok[l]; lv[l] = l < P ? v[l] : __builtin_nan(""); lp[l] = has ? l : -1; ln[l] = has ? 1 : 0; }
    for (int o = 1; o < 64; o <<= 1) {
        double nv[64]; int np[64], nn[64];
        for (int l = 0; l < 64; ++l) {
            const double v2 = lv[l ^ o]; const int p2 = lp[l ^ o];
            nv[l] = lv[l]; np[l] = lp[l];
            if (sel_before(v2, p2, lv[l], lp[l])) { nv[l] = v2; np[l] = p2; }
            nn[l] = ln[l] + ln[l ^ o];
        }
        memcpy(lv, nv, sizeof lv); memcpy(lp, np, sizeof lp); memcpy(ln, nn, sizeof ln);
    }
    for (int l = 1; l < 64; ++l)
        if (lp[l] != lp[0] || ln[l] != ln[0] || (lp[0] >= 0 && !same(lv[l], lv[0]))) { printf("FAIL the lanes of the butterfly disagree (P = %d, lane %d)\n", P, l); ++failures; }
    score = lp[0] >= 0 ? lv[0] : __builtin_nan("");
    n_adm = ln[0];
    return lp[0];
}

static void run(int P, int G, int L, int S, Fill fill, int obj_kind, int n_cons, int min_complete, bool none)
{
    const size_t GL = (size_t)G * L;
    if (none) min_complete = S + 1;      /* more complete realisations than there are: nobody is admissible */
    SelRule rule{};
    rule.obj = SelStat{(int)(rnd() % G), obj_kind, obj_kind >= SEL_QUANTILE ? (int)(rnd() % L) : 0};
    rule.n_cons = n_cons; rule.min_complete = min_complete;
    for (int k = 0; k < n_cons; ++k) {
        const int kind = L ? (int)(rnd() % SEL_N_KIND) : (int)(rnd() % SEL_QUANTILE);
        rule.cons[k] = SelStat{(int)(rnd() % G), kind, kind >= SEL_QUANTILE ? (int)(rnd() % L) : 0};
        rule.bound[k] = fill == SPECIAL && k % 3 == 1 ? (double)__builtin_inf() : 0.5;
    }
    std::vector<double> val(P), want_val(P);
    std::vector<unsigned char> ok(P), want_ok(P);
    for (int p = 0; p < P; ++p) {
        /* one candidate's risk, each array its own allocation of exactly the length the rule may read */
        std::vector<double> mean(G), mn(G), mx(G), qu(GL), hi(GL), lo(GL);
        std::vector<int> ex(G), counts(4);
        for (int j = 0; j < G; ++j) { mean[j] = draw(fill); mn[j] = draw(fill); mx[j] = draw(fill); ex[j] = fill == TIED ? 1 : (int)(rnd() % 3); }
        for (size_t o = 0; o < GL; ++o) { qu[o] = draw(fill); hi[o] = draw(fill); lo[o] = draw(fill); }
        counts[0] = (int)(rnd() % (S + 1)); counts[1] = S - counts[0]; counts[2] = counts[3] = 0;
        SelRisk R{};
        R.L = L; R.mean = mean.data(); R.min = mn.data(); R.max = mx.data(); R.n_exceed = ex.data();
        R.quantile = L ? qu.data() : nullptr; R.cvar_hi = L ? hi.data() : nullptr; R.cvar_lo = L ? lo.data() : nullptr; R.counts = counts.data();
        double score = -7.0;
        ok[p] = sel_admissible(R, rule, score) ? 1 : 0;
        val[p] = score;
        /* the restatement */
        auto value = [&](const SelStat &s) -> double {
            if (s.kind == 0) return mean[s.col];
            if (s.kind == 1) return mn[s.col];
            if (s.kind == 2) return mx[s.col];
            if (s.kind == 3) return (double)ex[s.col];
            const size_t o = (size_t)s.col * L + s.lvl;
            return s.kind == 4 ? qu[o] : s.kind == 5 ? hi[o] : lo[o];
        };
        want_val[p] = value(rule.obj);
        bool adm = counts[0] >= min_complete && !isnan(want_val[p]);
        for (int k = 0; k < n_cons; ++k) { const double c = value(rule.cons[k]); if (isnan(c) || !(c <= rule.bound[k])) adm = false; }
        want_ok[p] = adm ? 1 : 0;
        if (!same(val[p], want_val[p])) fail("value", P, p, val[p], want_val[p]);
        if (ok[p] != want_ok[p]) fail("admissible", P, p, ok[p], want_ok[p]);
    }
    int want = -1, want_n = 0;
    for (int p = 0; p < P; ++p) {
        if (!want_ok[p]) continue;
        ++want_n;
        if (want < 0 || want_val[p] < want_val[want]) want = p;      /* the first least value: strict <, so -0.0 does not beat +0.0 */
    }
    const double want_score = want >= 0 ? want_val[want] : __builtin_nan("");
    double s1 = -7.0, s2 = -7.0; int n1 = -7, n2 = -7;
    const int c1 = sel_scan(val.data(), ok.data(), P, s1, n1), c2 = butterfly(val.data(), ok.data(), P, s2, n2);
    if (c1 != want) fail("choice (serial scan)", P, -1, c1, want);
    if (c2 != want) fail("choice (butterfly)", P, -1, c2, want);
    if (!same(s1, want_score)) fail("score (serial scan)", P, -1, s1, want_score);
    if (!same(s2, want_score)) fail("score (butterfly)", P, -1, s2, want_score);
    if (n1 != want_n) fail("n_admissible (serial scan)", P, -1, n1, want_n);
    if (n2 != want_n) fail("n_admissible (butterfly)", P, -1, n2, want_n);
    if (none && want != -1) fail("nobody admissible, yet a choice", P, -1, want, -1);
}

int main()
{
    /* THE ORDER's corners */
    const double nanv = __builtin_nan("");
    if (!sel_before(0.0, 0, 1.0, 1) || sel_before(1.0, 0, 0.0, 1) || !sel_before(0.0, 1, -0.0, 2) || sel_before(-0.0, 2, 0.0, 1) || sel_before(0.0, -1, 1.0, 3) ||
        !sel_before(1.0, 3, nanv, -1) || sel_before(nanv, -1, nanv, -1)) { printf("FAIL sel_before\n"); ++failures; }
    int runs = 0;
    for (int P = 1; P <= 64; ++P)
        for (int fill = 0; fill < 3; ++fill)
            for (int kind = 0; kind < SEL_N_KIND; ++kind) {
                run(P, 5, 3, 4, (Fill)fill, kind, 0, 4, false); ++runs;
                run(P, 64, 8, 64, (Fill)fill, kind, 8, 1, false); ++runs;
                run(P, 1, 1, 1, (Fill)fill, kind, 1, 1, false); ++runs;
                run(P, 3, 2, 2, (Fill)fill, kind, 1, 1, true); ++runs;      /* nobody admissible, with a constraint */
                run(P, 3, 2, 2, (Fill)fill, kind, 0, 1, true); ++runs;      /* ... and without */
                if (kind < SEL_QUANTILE) { run(P, 2, 0, 3, (Fill)fill, kind, 1, 2, false); ++runs; }      /* L = 0: no per-level array exists */
            }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("plan select host check: %d instances, every choice as the naive restatement gives it\n", runs);
    return 0;
}
