"""Fallback inputs for instances of a resident batch whose solve left no usable plan (mld_sim_step_fallback, GpuProblem.sim_step(resolve=R, fallback=...)).

The reference never freezes a plant: solve_grid_mpc catches the solver's error, warns "Using last solution, will not be optimal" and goes on
(examples/residential_mg_with_pv_and_dewhs/modelling/micro_grid_agents.py:728-735), and sim_step_k steps the plant with whatever variables_k.u holds
(controllers/controller_base.py:229-253).  The device chooses the source of u per instance, the first that applies:

    0  PLAN     the plan is usable                              the plan's step-0 input
    1  MEMORY   "memory" allowed and 1 <= age <= N_tilde - 1    mem_u[b, age]: the row the remembered plan made for the current time
    2  POLICY   "policy" allowed                                the resident policy's rule on x and u_prev (policy.apply_np)
   -1  NONE     none of them                                    the instance is not attempted (its u below is 0)

and after an advancing step a usable plan becomes the memory (age 1), while any other source makes a remembered plan one step older (age N_tilde =
exhausted, -1 = nothing remembered stays -1).  `choose_np` and `commit_np` restate the two rules in numpy, as policy.apply_np restates the thermostat.
(The reference re-applies the stale plan's step-0 input; the row for the current time is the receding-horizon-consistent choice.)
"""
import numpy as np

from . import policy as _policy

PLAN, MEMORY, POLICY, NONE = 0, 1, 2, -1
FB_BITS = dict(memory=1, policy=2)      # MLD_FB_MEMORY, MLD_FB_POLICY


def fb_bits(fallback):
    """the fb argument of mld_sim_step_fallback from an int or from names: any subset of ("memory", "policy")"""
    if isinstance(fallback, (int, np.integer)):
        return int(fallback)
    if isinstance(fallback, str):
        fallback = (fallback,)
    fb = 0
    for name in fallback:
        if name not in FB_BITS:
            raise ValueError("fallback source %r is not one of %s" % (name, sorted(FB_BITS)))
        fb |= FB_BITS[name]
    return fb


def choose_np(usable, plan_u, mem_u, age, fb, P=None, midx=None, x=None, u_prev=None):
    """the source and the input of one fallback step: usable (B,) bool, plan_u (B, nu) the plans' step-0 inputs (read only where usable), mem_u
    (B, N, nu) and age (B,) the plan memory (None: none enabled), fb the allowed sources (int bits or names); for the policy P a
    policy.ThresholdPolicy with midx (B,) or None, x (B, nx) and u_prev (B, nu).  Returns (u (B, nu), source (B,) int32)."""
    fb = fb_bits(fb)
    usable = np.asarray(usable, dtype=bool)
    B = usable.shape[0]
    plan_u = np.asarray(plan_u, dtype=np.float64).reshape(B, -1)
    nu = plan_u.shape[1]
    source = np.full(B, NONE, np.int32)
    u = np.zeros((B, nu))
    if fb & FB_BITS["policy"]:
        if P is None or x is None or u_prev is None:
            raise ValueError("the policy source needs P, x and u_prev")
        if not P.all_ruled:
            raise ValueError("the policy passes a channel through: an instance without a usable plan has no u such a channel could take")
        source[:] = POLICY
        u = _policy.apply_np(P, midx, x, u_prev)
    if fb & FB_BITS["memory"]:
        if mem_u is None or age is None:
            raise ValueError("the memory source needs mem_u and age")
        mem_u = np.asarray(mem_u, dtype=np.float64)
        age = np.asarray(age)
        N = mem_u.shape[1]
        held = (age >= 1) & (age <= N - 1)
        source[held] = MEMORY
        u = np.where(held[:, None], mem_u[np.arange(B), np.where(held, age, 0)], u)
    source[usable] = PLAN
    u = np.where(usable[:, None], plan_u, u)
    return np.ascontiguousarray(u), source


def commit_np(source, plan_u_all, mem_u, age, N):
    """the plan memory after an advancing step: source (B,) of choose_np, plan_u_all (B, N, nu) the plans' inputs of every step (read only where the
    source is PLAN), mem_u (B, N, nu), age (B,).  Returns new (mem_u, age (int32)); the arguments are left as they are."""
    source = np.asarray(source)
    B = source.shape[0]
    mem_u = np.array(mem_u, dtype=np.float64).reshape(B, N, -1)
    age = np.array(age, dtype=np.int32)
    plan = source == PLAN
    mem_u[plan] = np.asarray(plan_u_all, dtype=np.float64).reshape(mem_u.shape)[plan]
    older = ~plan & (age >= 1)
    age[older] = np.minimum(age[older] + 1, N)
    age[plan] = 1
    return mem_u, age


# ---- applying a kept selection (mld_sim_step_selected, GpuProblem.sim_step(resolve=R, selected=True)) ----------------------------------------------------
# The selection is the FIRST source, in place of the plan:
#     3  SELECTED   choice >= 0                                     sel_u[b, 0]: step 0 of the chosen sequence, or the chosen rule's step 0
#     1  MEMORY, 2  POLICY, -1  NONE                                as above
# The plan is deliberately not a source: the filter judged it or the caller left it out.  After an advancing step a plan or sequence pick (policy < 0) of
# K == N_tilde steps becomes the memory (age 1); every other instance ages as a non-plan source does, and with K != N_tilde nothing is remembered (the
# memory's rows are the time slots of a full horizon).
SELECTED = 3


def choose_selected_np(choice, sel_u, mem_u, age, fb, P=None, midx=None, x=None, u_prev=None):
    """the source, the input and the pick of one selected step: choice (B,) ints, -1 = none; sel_u (B, K, nu) the kept selection's inputs (row 0 read
    where choice >= 0); mem_u, age, fb, P, midx, x, u_prev as choose_np's.  Returns (u (B, nu), source (B,) int32, pick (B,) int32: the choice where the
    source is SELECTED, -1 elsewhere)."""
    choice = np.asarray(choice)
    if choice.ndim != 1 or not np.issubdtype(choice.dtype, np.integer):
        raise ValueError("choice has shape %s and dtype %s, expected (B,) integers" % (choice.shape, choice.dtype))
    B = choice.shape[0]
    sel_u = np.asarray(sel_u, dtype=np.float64)
    if sel_u.ndim != 3 or sel_u.shape[0] != B or sel_u.shape[1] < 1:
        raise ValueError("sel_u has shape %s, expected (%d, K >= 1, nu)" % (sel_u.shape, B))
    if np.any(choice < -1):
        raise ValueError("choice of instance %d is %d (-1 = none, or a candidate >= 0)" % (int(np.flatnonzero(choice < -1)[0]), int(choice[choice < -1][0])))
    picked = choice >= 0
    if not np.all(np.isfinite(sel_u[picked, 0])):
        raise ValueError("sel_u of instance %d, step 0 is not finite" % int(np.flatnonzero(picked & ~np.isfinite(sel_u[:, 0]).all(axis=1))[0]))
    u, source = choose_np(np.zeros(B, bool), np.zeros((B, sel_u.shape[2])), mem_u, age, fb, P=P, midx=midx, x=x, u_prev=u_prev)
    source[picked] = SELECTED
    u = np.where(picked[:, None], sel_u[:, 0], u)
    pick = np.where(picked, choice, -1).astype(np.int32)
    return np.ascontiguousarray(u), source, pick


def commit_selected_np(source, sel_policy, sel_u, mem_u, age, N):
    """the plan memory after an advancing selected step: source (B,) of choose_selected_np, sel_policy (B,) the kept selection's policy (-1: a plan or
    sequence pick), sel_u (B, K, nu), mem_u (B, N, nu), age (B,).  Returns new (mem_u, age (int32)); the arguments are left as they are."""
    source = np.asarray(source)
    B = source.shape[0]
    sel_policy = np.asarray(sel_policy)
    if sel_policy.shape != (B,):
        raise ValueError("sel_policy has shape %s, expected (%d,)" % (sel_policy.shape, B))
    sel_u = np.asarray(sel_u, dtype=np.float64)
    if sel_u.ndim != 3 or sel_u.shape[0] != B:
        raise ValueError("sel_u has shape %s, expected (%d, K, nu)" % (sel_u.shape, B))
    mem_u = np.array(mem_u, dtype=np.float64).reshape(B, N, -1)
    age = np.array(age, dtype=np.int32)
    kept = (source == SELECTED) & (sel_policy < 0) & (sel_u.shape[1] == N)
    if kept.any():
        mem_u[kept] = sel_u.reshape(mem_u.shape)[kept]
    older = ~kept & (age >= 1)
    age[older] = np.minimum(age[older] + 1, N)
    age[kept] = 1
    return mem_u, age
