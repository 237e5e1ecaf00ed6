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
