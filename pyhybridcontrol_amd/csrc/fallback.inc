// Fallback inputs of the resolving plant step (mld_sim_step_fallback): the reference never freezes a plant -- solve_grid_mpc catches the solver's error,
// warns "Using last solution, will not be optimal" and goes on (examples/residential_mg_with_pv_and_dewhs/modelling/micro_grid_agents.py:728-735), and
// sim_step_k steps the plant with whatever variables_k.u holds (controllers/controller_base.py:229-253).  Here an instance whose solve left no usable plan
// takes its u from the first source that applies:
//     0  PLAN     plan_usable(b)                                       the first nu entries of the resident plan's row
//     1  MEMORY   MLD_FB_MEMORY and 1 <= age[b] <= N_tilde - 1         mem_u[b, age[b], :]: the row the remembered plan made for NOW
//     2  POLICY   MLD_FB_POLICY                                        the resident policy's rule on x0[b] and u_prev[b] (policy_rule, the one copy)
//    -1  NONE     none of them                                         not attempted, as an instance without a usable plan is by mld_sim_step_resolve
// (the reference re-applies the stale plan's step-0 input; row age[b] is the receding-horizon-consistent choice).  Two kernels:
//   k_fallback_inputs   u (batch, nu), u_source (batch) and the attempt byte, into the buffers the resolving step's phases read     (before k_aux_inputs)
//   k_fallback_commit   after an advancing step: a usable plan's u of every step becomes the memory, age 1; any other source ages it (capped at N_tilde)
// The choice and the ageing are host-compilable functions (SM_HOST, as small_lds.inc) so that a stand-alone program can run them under the host sanitizers.
//
// Mapping, as k_profile_windows / k_aux_inputs: threads on DESTINATION elements (a wave's 64 stores are contiguous), the 64-bit split of the flat index
// into (instance, column) once per workgroup and iteration, the lanes finish it in 32 bits; workgroups stride over the batch.  Nothing is checked here: the
// host has validated every age (-1, 1 .. N_tilde) before it reached the device, and a memory row is read only for 1 <= age <= N_tilde - 1.
#pragma once

enum { FB_PLAN = 0, FB_MEMORY = 1, FB_POLICY = 2, FB_NONE = -1 };

// the source of instance b's u: usable = plan_usable(b), fb the MLD_FB_* bits of the call, age the memory's (-1 without one)
SM_FN int fb_source(bool usable, int fb, int age, int N)
{
    if (usable) return FB_PLAN;
    if ((fb & MLD_FB_MEMORY) && age >= 1 && age <= N - 1) return FB_MEMORY;
    if (fb & MLD_FB_POLICY) return FB_POLICY;
    return FB_NONE;
}

// the memory's age after an advancing step that took its u from `source`: a usable plan is remembered (1), anything else makes a remembered plan one
// step older, N = exhausted; nothing remembered (-1) stays so
SM_FN int fb_next_age(int source, int age, int N)
{
    if (source == FB_PLAN) return 1;
    return age >= 1 ? (age + 1 < N ? age + 1 : N) : age;
}

// u[b, j] by source.  plan_row: the resident plan's row of b; mem_row: mem_u[b] (N, nu); tab: channel j's policy row; x: x0[b]
SM_FN double fb_input(int source, int j, int nu, int nx, int age, const double *plan_row, const double *mem_row, const double *tab, const double *x, double prev)
{
    if (source == FB_PLAN) return plan_row[j];
    if (source == FB_MEMORY) return mem_row[(size_t)age * nu + j];
    if (source == FB_POLICY) return policy_rule(tab, nx, x, prev);
    return 0.0;      /* not attempted: the resolver never sees an unusable plan's garbage (as k_aux_inputs) */
}

#ifndef SM_HOST
struct FallbackArgs {
    int batch, nx, nu, nv, N, fb;
    const int *status; const double *obj;           /* the resident plan's */
    const double *v; size_t v_stride;               /* its rows (stride n), step k's u at k nv */
    double *mem_u; int *mem_age;                    /* (batch, N, nu), (batch); nullptr: no memory enabled, every age reads -1 */
    const int *model_idx; const double *tab; size_t tab_len; const double *x0, *u_prev;      /* the resident policy (read only where the source is POLICY) */
    double *u; int *source; unsigned char *attempt; /* (batch, nu), (batch), (batch): k_fallback_inputs writes, k_fallback_commit reads source */
};

__global__ void __launch_bounds__(256) k_fallback_inputs(const FallbackArgs a)
{
    const int W = a.nu;
    const long long total = (long long)a.batch * W;
    for (long long base = (long long)blockIdx.x * 256; base < total; base += (long long)gridDim.x * 256) {
        const long long b0 = base / W;                          // uniform over the workgroup
        unsigned c = (unsigned)(base - b0 * W) + threadIdx.x;
        const unsigned db = c / (unsigned)W;
        const long long b = b0 + db;
        c -= db * (unsigned)W;
        if (b >= a.batch) continue;
        const int age = a.mem_age ? a.mem_age[b] : -1;
        const int s = fb_source(plan_usable(a.status, a.obj, (int)b), a.fb, age, a.N);
        const double *tab = nullptr;
        double prev = 0.0;
        if (s == FB_POLICY) {
            tab = a.tab + (size_t)(a.model_idx ? a.model_idx[b] : 0) * a.tab_len + (size_t)c * (a.nx + POL_TAIL);
            prev = a.u_prev[b * a.nu + c];
        }
        const double *mem_row = a.mem_u ? a.mem_u + b * ((long long)a.N * a.nu) : nullptr;
        a.u[b * a.nu + c] = fb_input(s, (int)c, a.nu, a.nx, age, a.v + b * (long long)a.v_stride, mem_row, tab, a.x0 + b * a.nx, prev);
        if (c == 0) { a.source[b] = s; a.attempt[b] = s >= 0 ? 1 : 0; }
    }
}

// threads on the elements of mem_u; the plan's u of step k, channel j lies at row[k nv + j].  The thread of an instance's element 0 writes the age (no other
// thread of this kernel reads it).
__global__ void __launch_bounds__(256) k_fallback_commit(const FallbackArgs a)
{
    const int W = a.N * a.nu;
    const long long total = (long long)a.batch * W;
    for (long long base = (long long)blockIdx.x * 256; base < total; base += (long long)gridDim.x * 256) {
        const long long b0 = base / W;                          // uniform over the workgroup
        unsigned c = (unsigned)(base - b0 * W) + threadIdx.x;
        const unsigned db = c / (unsigned)W;
        const long long b = b0 + db;
        c -= db * (unsigned)W;
        if (b >= a.batch) continue;
        const int s = a.source[b];
        if (s == FB_PLAN) {
            const unsigned k = c / (unsigned)a.nu, j = c - k * (unsigned)a.nu;
            a.mem_u[b * W + c] = a.v[b * (long long)a.v_stride + (long long)k * a.nv + j];
        }
        if (c == 0) a.mem_age[b] = fb_next_age(s, a.mem_age[b], a.N);
    }
}
#endif
