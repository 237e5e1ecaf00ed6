// Resident disturbance profiles (mld_upload_profiles and its three consumers): every disturbance window the reference hands its controllers is a
// slice of a time series it holds once --
//   get_omega_tilde_k_hat / _act   profile.values[start:start + N_tilde].flatten()             (modelling/micro_grid_agents.py:236-298)
//   get_omega_tilde_scenario       scenarios.ravel(order='F')[flat_index : flat_index + N_tilde * nomega]                  (:206-232)
// -- so a window is (offset into a flat library, length).  The library lives in HBM, the windows are cut out there:
//     omega[k * nomega + j] = lib[s + (step + k) * width_g + (j - goff_g)]        k < N_tilde, j a channel of group g, s the start of group g
// One gather kernel writes the forecast of a batch, its extra constraint blocks, or a slice of validation columns.
//
// The destination is the large side (a gigabyte at the cfg4 shard with 20 columns), the library is small and re-read from cache: threads map to
// DESTINATION elements, a wave's 64 stores are 512 contiguous bytes.  A window row is a few hundred doubles, so a workgroup's 256 elements span at most
// a few rows: the 64-bit split of the flat index into (row, column) is done once per workgroup and iteration on the scalar unit, the lanes finish it
// with 32-bit arithmetic.  Nothing is checked here: the host has tested every start against the window rule before the launch (profile_check_starts).
#pragma once

#include <limits.h>

struct PfChan { int group, off, width; };      // per disturbance channel: its group, its offset inside the group, the group's width

#if defined(__HIPCC__)      /* (the window rule's test below also compiles for a host program without the HIP runtime: scripts/price_cost_host_check.cpp) */
// dst (rows, nW) contiguous, row r = (instance r / cols, column r % cols); that row's starts are start[((r / cols) * ld_cols + col0 + r % cols) * n_groups ..]:
// cols == ld_cols, col0 == 0 for a whole array, a slice of `cols` columns from col0 of ld_cols in the evaluate path.
__global__ void __launch_bounds__(256) k_profile_windows(int rows, int nW, int nomega, int cols, int ld_cols, int col0, int n_groups, const long long *start,
                                                         const PfChan *chan, int step, const double *lib, double *dst)
{
    const long long total = (long long)rows * nW;
    for (long long base = (long long)blockIdx.x * 256; base < total; base += (long long)gridDim.x * 256) {
        const int r0 = (int)(base / nW);                        // uniform over the workgroup
        unsigned c = (unsigned)(base - (long long)r0 * nW) + threadIdx.x;
        const unsigned dr = c / (unsigned)nW;
        const int r = r0 + (int)dr;
        c -= dr * (unsigned)nW;
        if (r >= rows) continue;
        const unsigned k = c / (unsigned)nomega, j = c - k * (unsigned)nomega;
        long long srow = r;
        if (cols != ld_cols) { const int b = r / cols; srow = (long long)b * ld_cols + col0 + (r - b * cols); }
        const PfChan ch = chan[j];
        const long long s = start[srow * n_groups + ch.group];
        dst[(long long)r * nW + c] = lib[s + (long long)(step + (int)k) * ch.width + ch.off];
    }
}
#endif

static int profile_grid(long long total)
{
    return (int)std::max<long long>(1, std::min<long long>((total + 255) / 256, 2048));      /* bounded: the rest is the grid-stride loop */
}

// the window rule's bounds test for one start: valid iff s >= 0 and s + (step + N) * width <= lib_len (written so that nothing overflows)
static inline bool profile_start_ok(long long s, long long lib_len, int step, int N, int width)
{
    return s >= 0 && s <= lib_len - ((long long)step + N) * (long long)width;
}
