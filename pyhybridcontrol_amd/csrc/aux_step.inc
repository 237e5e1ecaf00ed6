// The device-side path between a problem handle and its auxiliary resolver (mld_sim_step_resolve): the reference's closed loop steps the plant with u
// only -- ControllerBase.sim_step_k (controllers/controller_base.py:229-253) calls lsim_k(x_k=, u_k=, omega_k=), and MldModel.lsim_k (models/mld_model.py:
// 683-686) re-derives delta, z, mu under the REALISED omega_k by _compute_aux (:701-766) before it forms x_k1, y and cons.  The auxiliary problem is the
// horizon-1 instance of the solve path on the folded model (aux_resolve.py: u rides in the disturbance channel, omega' = [omega; u]), so two copy kernels are
// all that lies between the two handles:
//   k_aux_inputs   resolver.x0[b] = x[b],  resolver.omega[b] = [omega_used[b]; u[b]]           (before the resolver's solve)
//   k_aux_merge    v0[b] = [u[b]; resolver.v[b]] and the per-instance usable flag              (after it; k_sim_step then runs on v0 with the flag as mask)
// omega_used is the forecast's step 0 or one element run of the profile library (the window rule with ONE step, as k_sim_step reads it); u is the caller's
// (batch, nu) or the first nu entries of the resident plan's row.  An instance is ATTEMPTED when its u exists: always with the caller's u, with the plan's
// only where the plan is usable (plan_usable).  An instance that is not attempted gets u = 0 in the resolver -- the solve never sees an unusable plan's
// garbage -- and its result is discarded.
//
// Mapping, as k_profile_windows: threads on DESTINATION elements (a wave's 64 stores are contiguous inside a row's part), the 64-bit split of the flat index
// into (instance, column) once per workgroup and iteration, the lanes finish it in 32 bits; workgroups stride over the batch.  Nothing is checked here: the
// host has tested the starts against the window rule and the two handles' dimensions against each other before the launch.
#pragma once

struct AuxStepArgs {
    int batch, nx, nw, nu, nv, nv2, N;          /* the stepped problem's dims; nv2 = ndelta + nz + nmu, the resolver's row */
    const double *x0, *omega;                   /* its current inputs: (batch, nx), (batch, N nw) */
    const double *u; size_t u_stride;           /* the caller's (batch, nu), or the resident plan's rows (stride n) */
    const int *status; const double *obj;       /* the resident plan's, masking the instances whose u is not usable; nullptr = the caller's u, all attempted */
    const unsigned char *attempt;               /* nullptr: the rule above; else the attempt byte per instance itself (k_fallback_inputs: some source supplied its u) */
    const long long *act_start; const PfChan *chan; int n_groups, step; const double *lib;      /* act_start == nullptr: the forecast's step 0 */
    double *aux_x0, *aux_omega;                 /* k_aux_inputs writes: the resolver's inputs (batch, nx), (batch, nw + nu) */
    const double *aux_v; size_t aux_stride; const int *aux_status; const double *aux_obj;      /* k_aux_merge reads: the resolver's results (nullptr: nv2 == 0) */
    double *v0; unsigned char *usable; int *aux_status_out;      /* k_aux_merge writes: (batch, nv), (batch), (batch) */
};

__device__ __forceinline__ bool aux_attempted(const AuxStepArgs &a, int b) { return a.attempt ? a.attempt[b] != 0 : (!a.status || plan_usable(a.status, a.obj, b)); }

__global__ void __launch_bounds__(256) k_aux_inputs(const AuxStepArgs a)
{
    const int W = a.nx + a.nw + a.nu, nw2 = a.nw + a.nu;      /* a destination row: [x | omega_used | u] */
    const long long total = (long long)a.batch * W;
    for (long long base = (long long)blockIdx.x * 256; base < total; base += (long long)gridDim.x * 256) {
        const long long b0 = base / W;                          // uniform over the workgroup
        unsigned c = (unsigned)(base - b0 * W) + threadIdx.x;
        const unsigned db = c / (unsigned)W;
        const long long b = b0 + db;
        c -= db * (unsigned)W;
        if (b >= a.batch) continue;
        if (c < (unsigned)a.nx) { a.aux_x0[b * a.nx + c] = a.x0[b * a.nx + c]; continue; }
        const unsigned j = c - (unsigned)a.nx;
        double t;
        if (j < (unsigned)a.nw) {
            if (a.act_start) { const PfChan ch = a.chan[j]; t = a.lib[a.act_start[b * a.n_groups + ch.group] + (long long)a.step * ch.width + ch.off]; }
            else t = a.omega[b * ((long long)a.N * a.nw) + j];
        } else t = aux_attempted(a, (int)b) ? a.u[b * (long long)a.u_stride + (j - (unsigned)a.nw)] : 0.0;
        a.aux_omega[b * nw2 + j] = t;
    }
}

// usable = attempted AND the resolver left a feasible point (plan_usable on ITS results: OPTIMAL, or NODE_LIMIT with a finite objective -- all the reference
// asks of _compute_aux).  An unusable instance gets a NaN row, as the reference returns NaN auxiliaries there (:757-763).  aux_status_out: the resolver's
// status, 0 where there is nothing to resolve (nv2 == 0), -1 for an instance that was not attempted.  Binaries are copied as the solver returns them (0 / 1).
__global__ void __launch_bounds__(256) k_aux_merge(const AuxStepArgs a)
{
    const int W = a.nv > 0 ? a.nv : 1;                          /* one thread per instance even without a single input */
    const long long total = (long long)a.batch * W;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long base = (long long)blockIdx.x * 256; base < total; base += (long long)gridDim.x * 256) {
        const long long b0 = base / W;                          // uniform over the workgroup
        unsigned c = (unsigned)(base - b0 * W) + threadIdx.x;
        const unsigned db = c / (unsigned)W;
        const long long b = b0 + db;
        c -= db * (unsigned)W;
        if (b >= a.batch) continue;
        const bool tried = aux_attempted(a, (int)b);
        const bool ok = tried && (!a.nv2 || plan_usable(a.aux_status, a.aux_obj, (int)b));
        if (c < (unsigned)a.nv) {
            const double t = c < (unsigned)a.nu ? a.u[b * (long long)a.u_stride + c] : a.aux_v[b * (long long)a.aux_stride + (c - (unsigned)a.nu)];
            a.v0[b * a.nv + c] = ok ? t : qnan;
        }
        if (c == 0) {
            a.usable[b] = ok ? 1 : 0;
            a.aux_status_out[b] = tried ? (a.nv2 ? a.aux_status[b] : 0) : -1;
        }
    }
}
