// The byte rule of a MIP start taken from a rollout (mld_warm_start_from_rollout, kernel k_warm_from_rollout in kernels.inc): the reference hands its
// backend the previous values as a start (warm_start=True, controllers/controller_base.py:493,509-512); an instance without a usable plan has none, and
// takes the plan of a rolled-out baseline instead.  The rule of ONE element (instance b, binary k) is written once, as a host-compilable function (WS_FN),
// so that a stand-alone program runs it over the index edges under the host sanitizers (scripts/start_rollout_host_check.cpp) and the numpy statement
// (pyhybridcontrol_amd/simlog.py: start_from_rollout_np) has one text to agree with.
//   source of instance b    0 kept      a start is resident, the call keeps, and the row's first byte is not 255
//                           1 written   the trajectory ended complete: byte k = v[b, step, pos] > 0.5 ? 1 : 0, bins[k] = step nv + pos (a NaN rounds to 0)
//                          -1 / -2 / -3 the auxiliary problem of some step is infeasible / the LDS solver declined / not attempted: the whole row 255
// `old` is a COPY of the resident start taken before the launch (nullptr: nothing is kept): the keep test reads the row's first byte, which the thread of
// element (b, 0) writes -- read from the start itself, the threads of one row would race.
#pragma once

#if defined(__HIPCC__)
#define WS_FN __host__ __device__ inline
#else
#define WS_FN static inline
#endif

enum { WS_WRITTEN = 1, WS_KEPT = 0, WS_INFEASIBLE = -1, WS_DECLINED = -2, WS_NOT_ATTEMPTED = -3, WS_NONE = 255 };

// the source of an instance's row: end_status as k_rollout writes it (RO_COMPLETE 0, RO_INFEASIBLE 1, RO_DECLINED 2, RO_NOT_ATTEMPTED -1)
WS_FN int ws_source(int end_status, bool keep, unsigned char old_first)
{
    if (keep && old_first != WS_NONE) return WS_KEPT;
    return end_status == 0 ? WS_WRITTEN : (end_status == 1 ? WS_INFEASIBLE : (end_status == 2 ? WS_DECLINED : WS_NOT_ATTEMPTED));
}

// element t = b nb + k of the start: writes warm[t] unless the row is kept, returns the row's source.  v: the rollout's (batch, N_tilde, nv), row stride
// v_stride; end_status (batch); old: (batch, nb) or nullptr
WS_FN int ws_element(unsigned long long t, int nb, int nv, const int *bins, const double *v, size_t v_stride, const int *end_status, const unsigned char *old,
                     unsigned char *warm)
{
    const unsigned long long b = t / (unsigned)nb;
    const int k = (int)(t - b * (unsigned)nb);
    const int src = ws_source(end_status[b], old != nullptr, old ? old[b * (unsigned)nb] : (unsigned char)WS_NONE);
    if (src == WS_KEPT) return src;
    if (src != WS_WRITTEN) { warm[t] = WS_NONE; return src; }
    const int j = bins[k], step = j / nv, pos = j - step * nv;
    const double val = v[b * v_stride + (size_t)step * nv + pos];
    warm[t] = val > 0.5 ? 1 : 0;
    return src;
}
