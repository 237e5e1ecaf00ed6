// Host big-M tightening of one step model (per model, once, at mld_problem_create).
// ------------------------------------------------------------------------------------------------
// probing-based coefficient tightening of one step's MLD rows (Savelsbergh 1994, sections 1.1, 3.2-3.3).
// MLD models are big-M translations of logic; with loose constants the LP relaxation of the condensed
// problem is very weak.  Integer-feasible points are unchanged.  Works on W = [E F1 F2 F3 F4 G Psi].
// ------------------------------------------------------------------------------------------------
namespace tighten {
static const double INF = std::numeric_limits<double>::infinity();

static bool propagate(const std::vector<double> &W, const std::vector<double> &c, int nc, int nt, std::vector<double> &lb,
                      std::vector<double> &ub, const std::vector<char> &is_int)
{
    for (int pass = 0; pass < 6; ++pass) {
        bool changed = false;
        for (int i = 0; i < nc; ++i) {
            const double *a = &W[(size_t)i * nt];
            double tot = 0; int ninf = 0, jinf = -1, nnz = 0;
            for (int j = 0; j < nt; ++j) {
                if (a[j] == 0) continue;
                nnz++;
                const double lc = a[j] > 0 ? a[j] * lb[j] : a[j] * ub[j];
                if (std::isinf(lc)) { ninf++; jinf = j; } else tot += lc;
            }
            if (!nnz) continue;
            if (!ninf && tot > c[i] + 1e-9 * std::max(1.0, std::fabs(c[i]))) return false;
            if (ninf > 1) continue;
            for (int j = 0; j < nt; ++j) {
                if (a[j] == 0) continue;
                double rest;
                if (!ninf) rest = tot - (a[j] > 0 ? a[j] * lb[j] : a[j] * ub[j]);
                else if (j == jinf) rest = tot;
                else continue;
                double b = (c[i] - rest) / a[j];
                if (a[j] > 0) {
                    if (is_int[j]) b = std::floor(b + 1e-9);
                    if (b < ub[j] - 1e-12 * std::max(1.0, std::fabs(b))) { ub[j] = b; changed = true; }
                } else {
                    if (is_int[j]) b = std::ceil(b - 1e-9);
                    if (b > lb[j] + 1e-12 * std::max(1.0, std::fabs(b))) { lb[j] = b; changed = true; }
                }
            }
        }
        for (int j = 0; j < nt; ++j) if (lb[j] > ub[j] + 1e-9) return false;
        if (!changed) break;
    }
    return true;
}

static double max_activity(const double *a, int nt, const std::vector<double> &lb, const std::vector<double> &ub, int skip)
{
    double s = 0;
    for (int j = 0; j < nt; ++j) {
        if (j == skip || a[j] == 0) continue;
        s += a[j] > 0 ? a[j] * ub[j] : a[j] * lb[j];
    }
    return s;
}

// mats: 20 host matrices of ONE model (row-major); modifies E..Psi / f5 copies in place
static void run(const mld_dims &d, std::vector<std::vector<double>> &mats, size_t model, int rounds = 2)
{
    const int sizes[7] = {d.nx, d.nu, d.ndelta, d.nz, d.nomega, d.ny, d.nmu};
    const int ids[7] = {MT_E, MT_F1, MT_F2, MT_F3, MT_F4, MT_G, MT_Psi};
    int offs[8]; offs[0] = 0;
    for (int k = 0; k < 7; ++k) offs[k + 1] = offs[k] + sizes[k];
    const int nt = offs[7], nc = d.nc;
    if (!nc || !nt) return;
    std::vector<double> W((size_t)nc * nt, 0.0), c(nc, 0.0);
    for (int k = 0; k < 7; ++k)
        for (int i = 0; i < nc; ++i)
            for (int j = 0; j < sizes[k]; ++j)
                W[(size_t)i * nt + offs[k] + j] = mats[ids[k]][model * (size_t)nc * sizes[k] + (size_t)i * sizes[k] + j];
    for (int i = 0; i < nc; ++i) c[i] = mats[MT_f5][model * (size_t)nc + i];
    std::vector<double> lb(nt, -INF), ub(nt, INF);
    std::vector<char> is_int(nt, 0);
    std::vector<int> bins;
    for (int j = offs[1] + d.nu - d.nu_l; j < offs[1] + d.nu; ++j) bins.push_back(j);
    for (int j = offs[2]; j < offs[2] + d.ndelta; ++j) bins.push_back(j);
    for (int j = offs[6] + d.nmu - d.nmu_l; j < offs[6] + d.nmu; ++j) bins.push_back(j);
    for (int j = offs[6]; j < offs[6] + d.nmu; ++j) lb[j] = 0.0;          // mu >= 0 (variables.py:221)
    for (int j : bins) { lb[j] = 0; ub[j] = 1; is_int[j] = 1; }
    for (int rnd = 0; rnd < rounds; ++rnd) {
        if (!propagate(W, c, nc, nt, lb, ub, is_int)) return;           // rows infeasible on their own: leave alone
        const size_t nbn = bins.size();
        std::vector<std::vector<double>> cl(2 * nbn), cu(2 * nbn);
        std::vector<char> ok(2 * nbn, 0);
        for (size_t t = 0; t < nbn; ++t)
            for (int v = 0; v < 2; ++v) {
                const int b = bins[t];
                if (!(lb[b] <= v && v <= ub[b])) continue;
                cl[2 * t + v] = lb; cu[2 * t + v] = ub;
                cl[2 * t + v][b] = cu[2 * t + v][b] = v;
                ok[2 * t + v] = propagate(W, c, nc, nt, cl[2 * t + v], cu[2 * t + v], is_int);
            }
        for (size_t t = 0; t < nbn; ++t) {
            if (!ok[2 * t] && ok[2 * t + 1]) lb[bins[t]] = 1.0;
            else if (!ok[2 * t + 1] && ok[2 * t]) ub[bins[t]] = 0.0;
        }
        for (int i = 0; i < nc; ++i)
            for (size_t t = 0; t < nbn; ++t) {
                const int b = bins[t];
                double *a = &W[(size_t)i * nt];
                const double ab = a[b];
                if (ab == 0.0) continue;
                if (ab > 0) {                    // b = 0 side: rest <= c_i
                    if (!ok[2 * t]) continue;
                    const double U = max_activity(a, nt, cl[2 * t], cu[2 * t], b);
                    if (std::isfinite(U) && U < c[i] - 1e-12 * std::max(1.0, std::fabs(c[i]))) { const double dl = c[i] - U; c[i] = U; a[b] = ab - dl; }
                } else {                         // b = 1 side: rest <= c_i - a_b
                    if (!ok[2 * t + 1]) continue;
                    const double U = max_activity(a, nt, cl[2 * t + 1], cu[2 * t + 1], b);
                    if (std::isfinite(U) && U < c[i] - ab - 1e-12 * std::max(1.0, std::fabs(c[i] - ab))) a[b] = c[i] - U;
                }
            }
    }
    for (int k = 0; k < 7; ++k)
        for (int i = 0; i < nc; ++i)
            for (int j = 0; j < sizes[k]; ++j)
                mats[ids[k]][model * (size_t)nc * sizes[k] + (size_t)i * sizes[k] + j] = W[(size_t)i * nt + offs[k] + j];
    for (int i = 0; i < nc; ++i) mats[MT_f5][model * (size_t)nc + i] = c[i];
}
} // namespace tighten
