// k_small_milp: small MILPs solved ENTIRELY IN LDS, one 64-lane wave per instance (opt-in: MLD_SMALL_LDS, decided per problem in
// mld_problem_create).  The regime is the other end of k_solve's: problems whose whole dense dictionary is a few KB -- the horizon-1
// auxiliary problems of mld_sim_step_resolve (16 unknowns, 20 rows), short-horizon controllers -- for which a 512-thread workgroup, a
// dictionary in HBM, presolve, cuts and a dozen block barriers per pivot are all overhead.
//
// It reads exactly what k_solve reads for the instance (ProblemDev: Gs by model, qs, lb, ub, bins, cs, the constant's maps; BatchDev: hs,
// qs_inst / rconst, fixed), so its answer is the answer to the same scaled, tightened problem.  The algorithm is the textbook core of
// oracle/mld_oracle.c and problem.inc without their large-problem machinery:
//   * bounded dual simplex on a dense dictionary x_B = beta - D x_N with the reduced-cost row as its last row, started from the slack basis;
//     Harris two-pass ratio test with k_solve's tolerances; Bland's rule (smallest variable on both sides) after 30 pivots without progress;
//   * free continuous variables as k_solve has them: boxed at +-S_BIG only while non-basic (lo / hi keep the true bounds, xN the resting value);
//   * depth-first branch-and-bound on the one dictionary by bound changes, most fractional binary, nearest side first, nodes pruned
//     against the incumbent with gap_abs / gap_rel; every integral point is checked against the ORIGINAL rows before it becomes the incumbent.
// No cuts, no presolve, no devex, no perturbation, no refactorisation.  It must be right when it answers and it may DECLINE (status -1 and
// one device counter): pivot or node budget spent, a pivot below S_PIV_TINY, a row that can neither be repaired nor proven infeasible, an
// integral point that fails the residual check at S_RESID_TOL, a free variable resting on the artificial box.  The host re-solves what it
// declined with k_solve (api_solve.inc, launch_small), so NODE_LIMIT / NUMERICAL / UNBOUNDED stay k_solve's to report.
//
// Mapping: SM_WAVES waves per workgroup, each with a private region of the dynamic LDS block (SmShape::wave_doubles doubles) and its own
// instances from the problem's atomic counter.  The waves of a workgroup share nothing and the kernel holds no __syncthreads; lanes hand
// values over through LDS between wavefront-scope fences (sm_sync).  Every reduction is a butterfly whose result does not depend on the lane
// order, every tie is broken by index: an instance's bits do not depend on the batch, its position or the wave that took it.
// Rows and columns are looped (lane, lane + 64, ...): nothing assumes m + 1 <= 64 or n + 1 <= 64.
//
// The solver core (sm_solve and below) also compiles for the host: with SM_HOST defined a "wave" is one lane, the LDS block is plain memory
// and the fences are empty, so a stand-alone program with its own main can run the core under the host sanitizers (include mldgpu.h, define SM_HOST,
// include this file, give sm_solve a buffer of exactly sm_wave_doubles() doubles).
#pragma once

#ifdef SM_HOST
#include <math.h>
#include <stdint.h>
#define SM_W 1
#define SM_FN static inline
typedef double sm_f64;
typedef int sm_i32;
#define S_BIG 1.0e7
#define S_PTOL 1e-8
#define S_PTOL_SKIP 1e-6
#define S_DTOL 1e-9
#define S_PIV_ABS 1e-7
#define S_PIV_REL 1e-7
#define S_PIV_TINY 1e-5
#define S_INTTOL 1e-6
#define S_COEF_ZERO 1e-9
#define S_RESID_TOL 1e-6
#define S_INF (__builtin_huge_val())
SM_FN void sm_sync() {}
SM_FN double sm_xor_f64(double v, int) { return v; }
SM_FN int sm_xor_i32(int v, int) { return v; }
SM_FN int sm_uniform(int v) { return v; }
#else
#define SM_W 64
#define SM_FN __device__ __forceinline__
typedef __attribute__((address_space(3))) double sm_f64;
typedef __attribute__((address_space(3))) int sm_i32;
// hand-over of LDS values between the lanes of ONE wave: its LDS instructions execute in order, so the fences only pin the compiler
SM_FN void sm_sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
SM_FN double sm_xor_f64(double v, int o) { return __shfl_xor(v, o, 64); }
SM_FN int sm_xor_i32(int v, int o) { return __shfl_xor(v, o, 64); }
SM_FN int sm_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
#endif

#define SM_WAVES 4                     // waves per workgroup
#define SM_NT (64 * SM_WAVES)
#define SM_WAVE_BUDGET (16 * 1024)     // bytes of LDS a wave may use: what decides eligibility (mld_problem_create)
#define SM_STALL 30                    // pivots without progress of the dual objective before Bland's rule takes over
#define SM_NONE 0x7fffffff

struct SmShape {
    int n, m, ld, nb, nx, nW;          // ld: odd row stride of the dictionary (column walks without bank conflicts)
    int cp, cshift;                    // lanes across a dictionary row (power of two <= wave size) and its log2
    int max_nodes, max_pivots;
    double gap_abs, gap_rel;
    int wave_doubles;                  // doubles of LDS per wave (sm_wave_doubles)
};

// doubles a wave needs: dictionary with the cost row, xB, xN, lo, hi, the staged pivot column and row; then the int arrays (basic, nonbasic, at_upper, pos, stack)
static inline size_t sm_wave_doubles(int n, int m, int nb)
{
    const size_t ld = (size_t)n | 1;
    const size_t dbl = (size_t)(m + 1) * ld + (size_t)m + n + n + n + (size_t)(m + 1) + n;
    const size_t ints = (size_t)m + n + n + (size_t)(n + m) + 2 * ((size_t)nb + 1);
    return (dbl + (ints + 1) / 2 + 1) & ~(size_t)1;
}

// what the core reads and writes for one instance (global memory on the device)
struct SmArgs {
    const double *G, *h, *q, *lb, *ub, *cs;      // m x n scaled rows, m right-hand sides, n scaled cost, bounds, column scales
    const unsigned char *is_int;                 // n
    const int *bins;                             // nb
    const unsigned char *fixed;                  // nb (255 = free) or null
    double *v_out;                               // n: the incumbent, unscaled
};
struct SmResult { double obj, lbnd; int status, nodes, pivots; };      // status -1: declined; obj / lbnd without the objective constant

struct SmWave {      // a wave's region of LDS
    sm_f64 *D, *xB, *xN, *lo, *hi, *col, *arow;
    sm_i32 *basic, *nonbasic, *atup, *pos, *stk_j, *stk_s;      // pos[var]: >= 0 its non-basic column, < 0 its row as ~row; stk_s: bit 0 first value, bit 1 second side taken
};

SM_FN double sm_wave_max(double v) { for (int o = SM_W / 2; o > 0; o >>= 1) v = fmax(v, sm_xor_f64(v, o)); return v; }
SM_FN double sm_wave_min(double v) { for (int o = SM_W / 2; o > 0; o >>= 1) v = fmin(v, sm_xor_f64(v, o)); return v; }
SM_FN double sm_wave_sum(double v) { for (int o = SM_W / 2; o > 0; o >>= 1) v += sm_xor_f64(v, o); return v; }
SM_FN int sm_wave_imin(int v) { for (int o = SM_W / 2; o > 0; o >>= 1) { const int v2 = sm_xor_i32(v, o); v = v2 < v ? v2 : v; } return sm_uniform(v); }
// largest value, smallest index among equals (idx SM_NONE: no candidate); the payload travels with the winner
SM_FN int sm_wave_argmax(double v, int idx, int &pay)
{
    for (int o = SM_W / 2; o > 0; o >>= 1) {
        const double v2 = sm_xor_f64(v, o); const int i2 = sm_xor_i32(idx, o), p2 = sm_xor_i32(pay, o);
        if (i2 != SM_NONE && (idx == SM_NONE || v2 > v || (v2 == v && i2 < idx))) { v = v2; idx = i2; pay = p2; }
    }
    pay = sm_uniform(pay);
    return sm_uniform(idx);
}

// new bounds of structural j (a binary of the search): a non-basic one moves to the bound its reduced cost asks for, the basic values follow
SM_FN void sm_set_bounds(const SmShape &S, const SmWave &w, int lane, int j, double l, double u)
{
    sm_sync();
    const int c = w.pos[j];
    double delta = 0.0, target = 0.0;
    if (c >= 0) { target = l == u ? l : (w.D[S.m * S.ld + c] >= 0.0 ? l : u); delta = target - w.xN[c]; }
    sm_sync();
    if (lane == 0) { w.lo[j] = l; w.hi[j] = u; if (c >= 0) { w.xN[c] = target; w.atup[c] = (l != u && target == u) ? 1 : 0; } }
    if (c >= 0 && delta != 0.0) for (int i = lane; i < S.m; i += SM_W) w.xB[i] -= w.D[i * S.ld + c] * delta;
    sm_sync();
}

enum { SM_LP_OPTIMAL = 0, SM_LP_INFEASIBLE = 1, SM_LP_DECLINE = 2 };

// bounded dual simplex from the current (dual feasible) dictionary
SM_FN int sm_dual_simplex(const SmShape &S, const SmWave &w, int lane, int &pivots)
{
    const int n = S.n, m = S.m, ld = S.ld;
    const int lc = lane & (S.cp - 1), lr = lane >> S.cshift, rp = SM_W >> S.cshift;
    int stall = 0;
    for (;;) {
        sm_sync();
        const bool bland = stall > SM_STALL;
        // ---- leaving row: largest bound violation (Bland: smallest variable among the violated)
        double bv = 0.0; int bi = SM_NONE, brow = -1;
        for (int i = lane; i < m; i += SM_W) {
            const int var = w.basic[i];
            const double x = w.xB[i], l = var < n ? w.lo[var] : 0.0, u = var < n ? w.hi[var] : S_INF;
            const double v = fmax(l - x, x - u);
            if (!(v > S_PTOL)) continue;
            const int key = bland ? var : i;
            if (bland ? key < bi : (bi == SM_NONE || v > bv)) { bv = v; bi = key; brow = i; }
        }
        int r;
        if (bland) { const int k = sm_wave_imin(bi); r = k == SM_NONE ? -1 : ~w.pos[k]; }
        else { r = sm_wave_argmax(bv, bi, brow) == SM_NONE ? -1 : brow; }
        if (r < 0) return SM_LP_OPTIMAL;
        if (pivots >= S.max_pivots) return SM_LP_DECLINE;
        const int lvar = w.basic[r];
        const double xl = w.xB[r], ll = lvar < n ? w.lo[lvar] : 0.0, lu = lvar < n ? w.hi[lvar] : S_INF;
        const bool below = ll - xl > xl - lu;
        const double viol = below ? ll - xl : xl - lu, leave_value = below ? ll : lu;
        // ---- ratio test over the row (Harris two-pass); a column is eligible when moving its variable off its bound repairs the row
        const sm_f64 *row = w.D + r * ld, *cost = w.D + m * ld;
        double emax = 0.0;
        for (int c = lane; c < n; c += SM_W) {
            const int var = w.nonbasic[c];
            if (var < n && w.lo[var] == w.hi[var]) continue;
            const double a = row[c]; const bool up = w.atup[c] != 0;
            if (below ? (up ? a > 0 : a < 0) : (up ? a < 0 : a > 0)) emax = fmax(emax, fabs(a));
        }
        emax = sm_wave_max(emax);
        const double ptol = fmax(S_PIV_ABS, S_PIV_REL * emax);
        double tmax = S_INF, rmin = S_INF, gain = 0.0;
        for (int c = lane; c < n; c += SM_W) {
            const int var = w.nonbasic[c];
            const double l = var < n ? w.lo[var] : 0.0, u = var < n ? w.hi[var] : S_INF;
            if (l == u) continue;
            const double a = row[c]; const bool up = w.atup[c] != 0;
            if (!(below ? (up ? a > 0 : a < 0) : (up ? a < 0 : a > 0))) continue;
            if (fabs(a) <= ptol) { if (fabs(a) > S_COEF_ZERO) gain += fabs(a) * (u - l); continue; }      // (what the entries too small to pivot on could still repair; below S_COEF_ZERO: rounding noise of a zero)
            const double da = fmax(up ? -cost[c] : cost[c], 0.0);
            tmax = fmin(tmax, (da + S_DTOL) / fabs(a)); rmin = fmin(rmin, da / fabs(a));
        }
        tmax = sm_wave_min(tmax);
        if (tmax == S_INF) {
            // no entry to pivot on: the row proves the node infeasible when even the small entries cannot close a clear violation
            gain = sm_wave_sum(gain);
            return (viol > S_PTOL_SKIP && gain < viol - S_PTOL_SKIP) ? SM_LP_INFEASIBLE : SM_LP_DECLINE;
        }
        rmin = sm_wave_min(rmin);
        double av = -1.0; int ai = SM_NONE, ac = -1;
        for (int c = lane; c < n; c += SM_W) {
            const int var = w.nonbasic[c];
            if (var < n && w.lo[var] == w.hi[var]) continue;
            const double a = row[c]; const bool up = w.atup[c] != 0;
            if (!(below ? (up ? a > 0 : a < 0) : (up ? a < 0 : a > 0)) || fabs(a) <= ptol) continue;
            const double ratio = fmax(up ? -cost[c] : cost[c], 0.0) / fabs(a);
            if (bland) { if (ratio <= rmin * (1 + 1e-12) + 1e-300 && var < ai) { ai = var; ac = c; } }
            else if (ratio <= tmax && (ai == SM_NONE || fabs(a) > av || (fabs(a) == av && var < ai))) { av = fabs(a); ai = var; ac = c; }
        }
        int q;
        if (bland) { const int k = sm_wave_imin(ai); q = k == SM_NONE ? -1 : w.pos[k]; }
        else { q = sm_wave_argmax(av, ai, ac) == SM_NONE ? -1 : ac; }
        if (q < 0) return SM_LP_DECLINE;
        const double aq = row[q];
        if (fabs(aq) < S_PIV_TINY) return SM_LP_DECLINE;
        const double dq = fmax(w.atup[q] ? -cost[q] : cost[q], 0.0);
        if (dq / fabs(aq) * viol > 1e-14) stall = 0; else stall++;
        // ---- stage the pivot column (every row's entry in column q, the cost row included) and the scaled pivot row
        const double inv = 1.0 / aq, theta = (xl - leave_value) * inv, enter_value = w.xN[q] + theta;
        const int evar = w.nonbasic[q];
        for (int i = lane; i <= m; i += SM_W) w.col[i] = w.D[i * ld + q];
        for (int c = lane; c < n; c += SM_W) w.arow[c] = c == q ? inv : row[c] * inv;
        sm_sync();
        // ---- values, then the dictionary: D'[i][c] = D[i][c] - D[i][q] a_c / a_q, column q = -D[i][q] / a_q, row r = a_c / a_q (1 / a_q in column q)
        for (int i = lane; i < m; i += SM_W) if (i != r) w.xB[i] -= w.col[i] * theta;
        for (int i = lr; i <= m; i += rp) {
            const double f = w.col[i];
            sm_f64 *di = w.D + i * ld;
            if (i == r) { for (int c = lc; c < n; c += S.cp) di[c] = w.arow[c]; }
            else if (f != 0.0) for (int c = lc; c < n; c += S.cp) di[c] = (c == q ? 0.0 : di[c]) - f * w.arow[c];
        }
        if (lane == 0) {
            w.xB[r] = enter_value; w.xN[q] = leave_value;
            w.basic[r] = evar; w.nonbasic[q] = lvar; w.pos[evar] = ~r; w.pos[lvar] = q;
            w.atup[q] = (!below && ll != lu) ? 1 : 0;
        }
        pivots++;
    }
}

// the structural values of the current vertex into arow[0 .. n) (binaries as they are)
SM_FN void sm_gather_x(const SmShape &S, const SmWave &w, int lane)
{
    sm_sync();
    for (int c = lane; c < S.n; c += SM_W) { const int var = w.nonbasic[c]; if (var < S.n) w.arow[var] = w.xN[c]; }
    for (int i = lane; i < S.m; i += SM_W) { const int var = w.basic[i]; if (var < S.n) w.arow[var] = w.xB[i]; }
    sm_sync();
}

SM_FN double sm_gtol(const SmShape &S, double v) { return fmax(S.gap_abs, S.gap_rel * fabs(v)); }

// One instance, start to finish.  mem: the wave's LDS region (S.wave_doubles doubles).
SM_FN void sm_solve(const SmShape &S, sm_f64 *mem, const SmArgs &A, int lane, SmResult &res)
{
    const int n = S.n, m = S.m, ld = S.ld, nb = S.nb;
    SmWave w;
    {
        sm_f64 *o = mem;
        w.D = o; o += (m + 1) * ld; w.xB = o; o += m; w.xN = o; o += n; w.lo = o; o += n; w.hi = o; o += n; w.col = o; o += m + 1; w.arow = o; o += n;
        sm_i32 *k = (sm_i32 *)o;
        w.basic = k; k += m; w.nonbasic = k; k += n; w.atup = k; k += n; w.pos = k; k += n + m; w.stk_j = k; k += nb + 1; w.stk_s = k;
    }
    res.status = -1; res.obj = S_INF; res.lbnd = -S_INF; res.nodes = 0; res.pivots = 0;
    // ---- slack basis: every structural non-basic at the bound its cost asks for, free variables resting on the artificial box
    for (int j = lane; j < n; j += SM_W) { w.lo[j] = A.lb[j]; w.hi[j] = A.ub[j]; A.v_out[j] = 0.0; }
    sm_sync();
    if (A.fixed) for (int k = lane; k < nb; k += SM_W) if (A.fixed[k] != 255) { const int j = A.bins[k]; w.lo[j] = w.hi[j] = (double)A.fixed[k]; }
    sm_sync();
    for (int e = lane; e < m * n; e += SM_W) { const int i = e / n, c = e - i * n; w.D[i * ld + c] = A.G[e]; }
    for (int c = lane; c < n; c += SM_W) {
        const double qc = A.q[c], l = w.lo[c], u = w.hi[c];
        w.D[m * ld + c] = qc;
        w.nonbasic[c] = c; w.pos[c] = c;
        if (l == u) { w.atup[c] = 0; w.xN[c] = l; }
        else if (qc >= 0) { w.atup[c] = 0; w.xN[c] = l == -S_INF ? -S_BIG : l; }
        else { w.atup[c] = 1; w.xN[c] = u == S_INF ? S_BIG : u; }
    }
    sm_sync();
    for (int i = lane; i < m; i += SM_W) {
        double a = A.h[i];
        for (int c = 0; c < n; ++c) a -= w.D[i * ld + c] * w.xN[c];
        w.xB[i] = a; w.basic[i] = n + i; w.pos[n + i] = ~i;
    }
    // ---- depth-first search
    double best = S_INF, root = -S_INF;
    bool have = false;
    int depth = 0, nodes = 0, pivots = 0;
    for (;;) {
        if (nodes >= S.max_nodes) { res.nodes = nodes; res.pivots = pivots; return; }      // declined
        nodes++;
        const int lp = sm_dual_simplex(S, w, lane, pivots);
        if (lp == SM_LP_DECLINE) { res.nodes = nodes; res.pivots = pivots; return; }
        bool open = false;
        if (lp == SM_LP_OPTIMAL) {
            sm_gather_x(S, w, lane);
            double part = 0.0;
            for (int j = lane; j < n; j += SM_W) part += A.q[j] * w.arow[j];
            const double ob = sm_wave_sum(part);
            if (nodes == 1) root = ob;
            if (!have || ob < best - sm_gtol(S, best)) {
                // most fractional basic binary (smallest index among equals)
                double fv = 0.0; int fj = SM_NONE, dummy = 0;
                for (int k = lane; k < nb; k += SM_W) {
                    const int j = A.bins[k];
                    const double f = fabs(w.arow[j] - rint(w.arow[j]));
                    if (f > S_INTTOL && (fj == SM_NONE || f > fv)) { fv = f; fj = j; }
                }
                const int bj = sm_wave_argmax(fv, fj, dummy);
                if (bj != SM_NONE) {
                    const int first = w.arow[bj] >= 0.5 ? 1 : 0;
                    if (lane == 0) { w.stk_j[depth] = bj; w.stk_s[depth] = first; }
                    depth++;
                    sm_set_bounds(S, w, lane, bj, (double)first, (double)first);
                    open = true;
                } else {
                    // integral: the rounded point against the original rows, then the incumbent
                    sm_sync();
                    for (int k = lane; k < nb; k += SM_W) { const int j = A.bins[k]; w.arow[j] = rint(w.arow[j]); }
                    sm_sync();
                    double worst = -S_INF, hit = 0.0, pob = 0.0;
                    for (int i = lane; i < m; i += SM_W) {
                        double acc = 0.0;
                        for (int c = 0; c < n; ++c) acc += A.G[i * n + c] * w.arow[c];
                        worst = fmax(worst, acc - A.h[i]);
                    }
                    for (int j = lane; j < n; j += SM_W) {
                        const double x = w.arow[j];
                        pob += A.q[j] * x;
                        worst = fmax(worst, fmax(w.lo[j] - x, x - w.hi[j]));
                        if (w.pos[j] >= 0 && ((A.lb[j] == -S_INF && x <= -0.999 * S_BIG) || (A.ub[j] == S_INF && x >= 0.999 * S_BIG))) hit = 1.0;
                    }
                    worst = sm_wave_max(worst); hit = sm_wave_max(hit); pob = sm_wave_sum(pob);
                    if (!(worst <= S_RESID_TOL) || hit > 0.0) { res.nodes = nodes; res.pivots = pivots; return; }      // declined
                    if (pob < best) {
                        best = pob; have = true;
                        for (int j = lane; j < n; j += SM_W) A.v_out[j] = w.arow[j] * A.cs[j];
                    }
                }
            }
        }
        if (open) continue;
        // ---- backtrack: levels whose second side is done are released, the deepest other one is flipped
        bool done = false;
        for (;;) {
            if (depth == 0) { done = true; break; }
            sm_sync();
            const int j = w.stk_j[depth - 1], s = w.stk_s[depth - 1];
            if (s & 2) { depth--; sm_set_bounds(S, w, lane, j, 0.0, 1.0); continue; }
            sm_sync();
            if (lane == 0) w.stk_s[depth - 1] = s | 2;
            const double v = (double)(1 - (s & 1));
            sm_set_bounds(S, w, lane, j, v, v);
            break;
        }
        if (done) break;
    }
    res.nodes = nodes; res.pivots = pivots;
    if (have) { res.status = MLD_STATUS_OPTIMAL; res.obj = best; res.lbnd = fmin(best, fmax(root, best - sm_gtol(S, best))); }
    else { res.status = MLD_STATUS_INFEASIBLE; res.obj = S_INF; res.lbnd = -S_INF; }
}

#ifndef SM_HOST
// A wave's next ticket of a work counter, uniform over the wave (k_small_milp's instances, k_rollout's trajectories).
// Every lane takes part in the claim (lane 0 adds 1, the others 0) behind a convergent barrier.  With `if (lane == 0) t = atomicAdd(...)` at the head
// of the work loop and an `if (lane == 0)` write-out at its end, the compiler threaded the other 63 lanes round the loop AHEAD of lane 0 (for them
// t is the constant 0): readfirstlane then read lane 1's zero, and the wave solved instance 0 for ever.
SM_FN int sm_claim(int *counter, int lane)
{
    sm_sync();
    return sm_uniform(atomicAdd(counter, lane == 0 ? 1 : 0));
}
SM_FN unsigned long long sm_claim(unsigned long long *counter, int lane)      // (the broadcast moves 32 bits: two halves)
{
    sm_sync();
    const unsigned long long t = atomicAdd(counter, lane == 0 ? 1ull : 0ull);
    return ((unsigned long long)(unsigned)sm_uniform((int)(t >> 32)) << 32) | (unsigned)sm_uniform((int)t);
}

__global__ void __launch_bounds__(SM_NT) k_small_milp(SmShape S, ProblemDev P, BatchDev B, int *declined)
{
    extern __shared__ double sm_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    sm_f64 *mem = (sm_f64 *)sm_lds + (size_t)wave * S.wave_doubles;
    const int n = S.n, m = S.m;
    for (;;) {
        const int inst = sm_claim(B.counter, lane);
        if (inst >= B.batch) break;
        const long long t_begin = wall_clock64();
        const int mdl = B.model_idx ? B.model_idx[inst] : 0;
        SmArgs A;
        A.G = P.Gs + (size_t)mdl * m * n; A.h = B.hs + (size_t)inst * m;
        A.q = B.qs_inst ? B.qs_inst + (size_t)inst * n : P.qs + (size_t)mdl * n;
        A.lb = P.lb + (size_t)mdl * n; A.ub = P.ub + (size_t)mdl * n; A.cs = P.cs + (size_t)mdl * n;
        A.is_int = P.is_int; A.bins = P.bins;
        A.fixed = B.fixed ? B.fixed + (size_t)inst * S.nb : nullptr;
        A.v_out = B.v_out + (size_t)inst * n;
        double part = 0.0;
        if (P.cx) for (int j = lane; j < S.nx; j += 64) part += P.cx[(size_t)mdl * S.nx + j] * B.x0[(size_t)inst * S.nx + j];
        if (P.cw) for (int j = lane; j < S.nW; j += 64) part += P.cw[(size_t)mdl * S.nW + j] * B.omega[(size_t)inst * S.nW + j];
        const double r_const = sm_wave_sum(part) + (P.c0 ? P.c0[mdl] : 0.0) + (B.rconst ? B.rconst[inst] : 0.0);
        SmResult res;
        sm_solve(S, mem, A, lane, res);
        if (res.status < 0) for (int j = lane; j < n; j += 64) A.v_out[j] = 0.0;
        if (lane == 0) {
            B.obj_out[inst] = res.status == MLD_STATUS_OPTIMAL ? res.obj + r_const : S_INF;
            B.lb_out[inst] = res.status == MLD_STATUS_OPTIMAL ? res.lbnd + r_const : -S_INF;
            B.status_out[inst] = res.status; B.nodes_out[inst] = res.nodes; B.pivots_out[inst] = res.pivots;
            B.ticks_out[inst] = wall_clock64() - t_begin;
            if (res.status < 0) atomicAdd(declined, 1);
        }
    }
}
#endif
