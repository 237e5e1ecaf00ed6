// The resolving plant step that applies a kept selection (mld_sim_step_selected): mld_rollout_select / mld_rollout_select_policy answer "which candidate
// should be applied now", and this step applies the answer where it lies -- the safety filter in front of the plant step (plan_select.inc), inside the loop
// that never leaves HBM.  An instance takes its u from the first source that applies:
//     3  SELECTED   choice[b] >= 0                                       sel_u[b, 0, :]: step 0 of the chosen sequence, or the chosen rule's step 0
//     1  MEMORY     MLD_FB_MEMORY and 1 <= age[b] <= N_tilde - 1         mem_u[b, age[b], :]                     (fb_source's rule, fallback.inc)
//     2  POLICY     MLD_FB_POLICY                                        the resident policy's rule              (fb_source's rule)
//    -1  NONE       none of them                                         not attempted
// The resident plan is NOT a source: the filter judged it (plan_first) or the caller left it out, so an instance without an admissible candidate goes to the
// memory or the policy -- that is what makes the filter a filter.  Two kernels beside k_fallback_inputs / k_fallback_commit, and one for the kept copy:
//   k_selected_inputs   u (batch, nu), u_source (batch), pick (batch) and the attempt byte, into the buffers the resolving step's phases read
//   k_selected_commit   after an advancing step: a chosen plan or sequence of K == N_tilde steps becomes the memory, age 1; anything else ages it.  The memory's
//                       rows are the time slots of a full horizon, so a sequence of K != N_tilde steps is not remembered (its instance ages like the others)
//   k_selection_policy  policy[b] of a kept selection from choice[b]: the candidates behind n_seq are the policies (queued behind k_plan_select)
// The rules are host-compilable functions (SM_HOST), fb_source / fb_input / fb_next_age reused where the rule is theirs; scripts/selected_host_check.cpp runs
// them under the host sanitizers.
//
// Mapping: k_fallback_inputs' and k_fallback_commit's -- threads on DESTINATION elements, the 64-bit split of the flat index once per workgroup and iteration,
// grid-stride.  Nothing is checked here: the host has validated choice, policy, K and every age before they reached the device; sel_u is read only where
// choice[b] >= 0 (row 0) or where the sequence is remembered (K == N_tilde rows, all finite by mld_set_selection's rule or copied whole by the select call).
#pragma once

enum { FB_SELECTED = 3 };

// the source of instance b's u: choice the kept selection's, fb the MLD_FB_* bits of the call, age the memory's (-1 without one)
SM_FN int sel_step_source(int choice, int fb, int age, int N)
{
    if (choice >= 0) return FB_SELECTED;
    return fb_source(false, fb, age, N);
}

// u[b, j] by source.  sel_row: sel_u[b] (K, nu), read at row 0 only; the others as fb_input's
SM_FN double sel_step_input(int source, int j, int nu, int nx, int age, const double *sel_row, const double *mem_row, const double *tab, const double *x, double prev)
{
    if (source == FB_SELECTED) return sel_row[j];
    return fb_input(source, j, nu, nx, age, nullptr, mem_row, tab, x, prev);
}

// what the log's pick array gets: the candidate applied, -1 where the source is another
SM_FN int sel_step_pick(int source, int choice) { return source == FB_SELECTED ? choice : -1; }

// is the applied sequence remembered?  A plan or sequence pick (policy < 0) of a full horizon; read from the SOURCE, not from the advanced mask (k_fallback_commit)
SM_FN bool sel_step_remembered(int source, int policy, int K, int N) { return source == FB_SELECTED && policy < 0 && K == N; }

// the memory's age after an advancing step: a remembered sequence counts as a usable plan does (1), anything else as a non-plan source (fb_next_age)
SM_FN int sel_step_next_age(int source, int policy, int K, int N, int age) { return fb_next_age(sel_step_remembered(source, policy, K, N) ? FB_PLAN : FB_NONE, age, N); }

// policy[b] of a kept selection: candidates [0, n_seq) are the plan and the sequences, the policies follow
SM_FN int sel_kept_policy(int choice, int n_seq) { return choice >= n_seq ? choice - n_seq : -1; }

#ifndef SM_HOST
struct SelectedArgs {
    int batch, nx, nu, N, fb, K;
    const int *choice, *policy; const double *sel_u; /* the kept selection: (batch), (batch), (batch, K, nu) */
    double *mem_u; int *mem_age;                     /* (batch, N, nu), (batch); nullptr: no memory enabled, every age reads -1 */
    const int *model_idx; const double *tab; size_t tab_len; const double *x0, *u_prev;      /* the resident policy (read only where the source is POLICY) */
    double *u; int *source, *pick; unsigned char *attempt;      /* (batch, nu), (batch) x 3: k_selected_inputs writes, k_selected_commit reads source */
};

__global__ void __launch_bounds__(256) k_selected_inputs(const SelectedArgs a)
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
        const int pick = a.choice[b];
        const int s = sel_step_source(pick, a.fb, age, a.N);
        const double *tab = nullptr;
        double prev = 0.0;
        if (s == FB_POLICY) {
            tab = a.tab + (size_t)(a.model_idx ? a.model_idx[b] : 0) * a.tab_len + (size_t)c * (a.nx + POL_TAIL);
            prev = a.u_prev[b * a.nu + c];
        }
        const double *mem_row = a.mem_u ? a.mem_u + b * ((long long)a.N * a.nu) : nullptr;
        a.u[b * a.nu + c] = sel_step_input(s, (int)c, a.nu, a.nx, age, a.sel_u + b * ((long long)a.K * a.nu), mem_row, tab, a.x0 + b * a.nx, prev);
        if (c == 0) { a.source[b] = s; a.pick[b] = sel_step_pick(s, pick); a.attempt[b] = s >= 0 ? 1 : 0; }
    }
}

// threads on the elements of mem_u; a remembered sequence has K == N rows, so element c of the instance's memory is element c of its sequence.  The thread of
// an instance's element 0 writes the age (no other thread of this kernel reads it).
__global__ void __launch_bounds__(256) k_selected_commit(const SelectedArgs a)
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
        const int s = a.source[b], pol = a.policy[b];
        if (sel_step_remembered(s, pol, a.K, a.N)) a.mem_u[b * W + c] = a.sel_u[b * W + c];
        if (c == 0) a.mem_age[b] = sel_step_next_age(s, pol, a.K, a.N, a.mem_age[b]);
    }
}

__global__ void __launch_bounds__(256) k_selection_policy(long long batch, int n_seq, const int *choice, int *policy)
{
    for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < batch; b += (long long)gridDim.x * 256) policy[b] = sel_kept_policy(choice[b], n_seq);
}
#endif
