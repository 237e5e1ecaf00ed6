"""Rule-based feedback policies (pyhybridcontrol_amd/policy.py, mld_upload_policy / mld_set_policy_state / mld_download_policy_state / mld_rollout_policy /
mld_sim_step_policy) at the boundary of the library and in numpy, without a GPU: header and binding agree, the options struct kept its size, the entry
points follow the conventions of their neighbours, the rule's table of cases, simlog.rollout_np(policy=...) against a loop over MldModel.lsim_k with
policy.apply_np, controllers.ThresholdController against the same loop, and every refusal of the constructor."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _rollout_ref
import pyhybridcontrol_amd as phc
from pyhybridcontrol_amd import _lib, policy, simlog, synthetic as syn
from pyhybridcontrol_amd.controllers import ThresholdController

HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mldgpu.h")).read()
NEW = dict(mld_upload_policy=7, mld_set_policy_state=2, mld_download_policy_state=2, mld_rollout_policy=24, mld_sim_step_policy=14)


def _args(name):
    m = re.search(r"int\s+%s\s*\(([^;]*?)\)\s*;" % name, HDR)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_and_binding_agree_on_the_prototypes():
    lib = _lib.load()
    for name, n in NEW.items():
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert len(_args(name)) == n == len(getattr(lib, name).argtypes), name
    assert [a.split("*")[-1].strip() for a in _args("mld_upload_policy")] == ["p", "sel", "on_at", "off_at", "u_on", "u_off", "mode"]
    ro, base = _args("mld_rollout_policy"), _args("mld_rollout_batch")
    assert ro[:5] == base[:5] and ro[5] == "const double *u_prev" and ro[6:22] == base[5:21]      # mld_rollout_batch's, u_prev behind u_seq ...
    assert ro[22] == "int32_t *switches_out" and ro[23] == base[21] == "int64_t stats[4]"          # ... and switches_out in front of stats
    assert len(base) == 22 and len(_lib.load().mld_rollout_batch.argtypes) == 22
    step, res = _args("mld_sim_step_policy"), _args("mld_sim_step_resolve")
    assert [a.split("*")[-1].split()[-1] for a in step[1:]] == [a.split("*")[-1].split()[-1] for a in res[1:]]
    assert "theromstat_control.py:38-64" in HDR and "controller_base.py:229-253" in HDR          # declared with the reference lines they replace


def test_opts_size_is_unchanged():
    assert int(_lib.load().mld_opts_size()) == C.sizeof(_lib.Opts) == 64


def test_entry_points_without_a_device_or_a_handle():
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    x, es, sw, stats, up = np.full(8, 7.0), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(4, 7, np.int64), np.full(3, 7.0)
    sel, col, mode = np.ones(9), np.ones(3), np.ones(3, np.int32)
    calls = (("mld_rollout_policy", lambda: lib.mld_rollout_policy(None, None, 2, 1, None, None, None, None, 0, None, 0, _lib.dptr(x), None, None, None, None, None, None,
                                                                   None, None, None, ip(es), ip(sw), stats.ctypes.data_as(C.POINTER(C.c_int64))), b"no batch resident"),
             ("mld_sim_step_policy", lambda: lib.mld_sim_step_policy(None, None, None, None, 0, 0, _lib.dptr(x), None, None, None, None, None, ip(es), ip(sw)), b"no batch resident"),
             ("mld_set_policy_state", lambda: lib.mld_set_policy_state(None, _lib.dptr(up)), b"no batch resident"),
             ("mld_download_policy_state", lambda: lib.mld_download_policy_state(None, _lib.dptr(up)), b"no batch resident"),
             ("mld_upload_policy", lambda: lib.mld_upload_policy(None, _lib.dptr(sel), _lib.dptr(col), _lib.dptr(col), _lib.dptr(col), _lib.dptr(col), ip(mode)), b"null problem"))
    for name, call, word in calls:
        rc = call()
        if _lib.device_count() < 1:
            assert rc == -2 and b"no HIP device" in lib.mld_last_error(), name           # MLD_ERR_NO_DEVICE, before anything else
        else:
            assert rc == -1 and word in lib.mld_last_error(), name                        # MLD_ERR_INVALID: no handle
    assert np.all(x == 7.0) and np.all(es == 7) and np.all(sw == 7) and np.all(stats == 7) and np.all(up == 7.0)


def test_apply_np_table_of_cases():
    """one channel on one state, on_at 50, off_at 60, u_on 2, u_off -1: the five regions, both equalities, a NaN, and on_at == off_at"""
    P = policy.ThresholdPolicy(np.ones((1, 1, 1)), 50.0, 60.0, u_on=2.0, u_off=-1.0)
    nan = np.nan
    table = [  # x, u_prev, u
        (49.0, -1.0, 2.0), (49.0, 2.0, 2.0),              # below the band: on
        (50.0, -1.0, 2.0),                                # s == on_at: on
        (55.0, 2.0, 2.0), (55.0, -1.0, -1.0),             # inside: holds
        (55.0, 1.0, -1.0), (55.0, 2.0 + 1e-15, -1.0),     # inside, u_prev is not EXACTLY u_on: off
        (60.0, 2.0, -1.0),                                # s == off_at: off
        (61.0, 2.0, -1.0), (61.0, -1.0, -1.0),            # above: off
        (nan, 2.0, 2.0), (nan, -1.0, -1.0),               # a NaN falls through to the comparison with u_prev
    ]
    x, up, want = (np.array(c, dtype=float).reshape(-1, 1) for c in zip(*table))
    assert np.array_equal(policy.apply_np(P, None, x, up), want)
    Q = policy.ThresholdPolicy(np.ones((1, 1, 1)), 55.0, 55.0, u_on=2.0, u_off=-1.0)
    x = np.array([[54.0], [55.0], [56.0], [55.0]]); up = np.array([[-1.0], [-1.0], [2.0], [2.0]])
    assert np.array_equal(policy.apply_np(Q, None, x, up), np.array([[2.0], [2.0], [-1.0], [2.0]]))      # at equality the first line wins
    # a passed-through channel, a selector over two states, a second model
    sel = np.zeros((2, 2, 2)); sel[:, 0] = 0.5; sel[:, 1, 1] = 1.0
    R = policy.ThresholdPolicy(sel, [[50.0, 0.0], [40.0, 0.0]], [[60.0, 0.0], [45.0, 0.0]], mode=[[1, 0], [1, 0]])
    assert not R.all_ruled and P.all_ruled
    u = policy.apply_np(R, np.array([0, 1, 1]), np.array([[40.0, 50.0], [40.0, 50.0], [30.0, 40.0]]), np.zeros((3, 2)), u_pass=np.array([[9.0, 7.0]] * 3))
    assert np.array_equal(u, np.array([[1.0, 7.0], [0.0, 7.0], [1.0, 7.0]]))             # s = 45: on for model 0 (<= 50), off for model 1 (>= 45); s = 35: on
    assert np.array_equal(R.initial_state(np.array([0, 1])), np.zeros((2, 2)))
    T = policy.ThresholdPolicy.thermostat(58.5, 61.5, 3, nx=4)
    assert T.sel.shape == (3, 4, 4) and np.array_equal(T.sel[1], np.eye(4)) and np.all(T.on_at == 58.5) and np.all(T.u_on == 1.0) and np.all(T.mode == 1)


def test_constructor_refusals():
    ok = dict(sel=np.ones((2, 3, 4)), on_at=np.zeros((2, 3)), off_at=np.ones((2, 3)))
    policy.ThresholdPolicy(**ok)
    bad = [("expected \\(n_models, nu, nx\\)", dict(sel=np.ones((3, 4)))),
           ("on_at has shape", dict(on_at=np.zeros((2, 4)))), ("off_at has shape", dict(off_at=np.zeros((3, 3)))),
           ("u_on has shape", dict(u_on=np.zeros(2))), ("u_off has shape", dict(u_off=np.zeros((2, 3, 1)))), ("mode has shape", dict(mode=np.ones((3, 2), int))),
           ("sel is not finite", dict(sel=np.where(np.arange(24).reshape(2, 3, 4) == 5, np.nan, 1.0))),
           ("on_at is not finite", dict(on_at=np.full((2, 3), -np.inf))), ("off_at is not finite", dict(off_at=np.full((2, 3), np.nan))),
           ("u_on is not finite", dict(u_on=np.inf)), ("u_off is not finite", dict(u_off=np.nan)),
           ("on_at > off_at for model 1, channel 2", dict(on_at=np.where(np.arange(6).reshape(2, 3) == 5, 1.5, 0.0))),
           ("other than 0", dict(mode=np.full((2, 3), 2))), ("other than 0", dict(mode=np.where(np.arange(6).reshape(2, 3) == 0, -1, 1)))]
    for match, kw in bad:
        with pytest.raises(ValueError, match=match):
            policy.ThresholdPolicy(**dict(ok, **kw))
    with pytest.raises(TypeError, match="ThresholdPolicy"):
        ThresholdController(dict(A=np.eye(1), B1=np.eye(1)), "thermo")


def _two_models(B, N, hard=False, tie=True):
    mats_list, models, xs, oms = [], [], [], []
    for k in range(2):
        rng = np.random.default_rng(8900 + k)
        mats, d, _ = syn.make_agent(3, rng, tie=tie)
        if hard:
            import _aux_ref
            mats, d = _aux_ref.hard_variant(mats, d)
        x0, om = syn.make_scenarios(3, N, B, rng, tie=tie)
        mats_list.append(mats); xs.append(x0); oms.append(om)
        models.append(phc.MldModel(nu_l=d["nu_l"], **mats))
    midx = np.arange(B) % 2
    return mats_list, models, d, midx, np.stack(xs)[midx, np.arange(B)], np.stack(oms)[midx, np.arange(B)]


def test_rollout_np_with_a_policy_equals_a_loop_over_lsim_k():
    """make_agent(3) x 2 models, 4 instances x 3 realisations x 12 steps of the thermostat, tank 2 passed through (mode 0, from u_seq); per step apply_np on
    the loop's own x and u_{k-1}, the closed form for delta, z, mu, MldModel.lsim_k for the step.  Every field is equal; without `policy` rollout_np returns
    what it returned (the same loop with u_seq itself)."""
    B, S, K, N = 4, 3, 12, 3
    mats_list, models, d, midx, x0, om = _two_models(B, N)
    nu = d["nu"]
    rng = np.random.default_rng(8910)
    u_seq = (rng.uniform(size=(B, K, nu)) < 0.4).astype(float)
    _, _, _, om_seq = _rollout_ref.realised_library(om, N, d["nomega"], d["nx"], S, K, 1, rng)
    fn = _rollout_ref.closed_form_resolver(mats_list, d)
    P = policy.ThresholdPolicy(np.broadcast_to(np.eye(3), (2, 3, 3)), 58.5, 61.5, mode=[1, 1, 0])
    u_prev = (rng.uniform(size=(B, nu)) < 0.5).astype(float)
    got = simlog.rollout_np(mats_list, d, midx, x0, u_seq, om_seq, fn, policy=P, u_prev=u_prev)
    plain = simlog.rollout_np(mats_list, d, midx, x0, u_seq, om_seq, fn)
    assert "switches" in got and "switches" not in plain and got["switches"].dtype == np.int32
    assert np.all(got["end_status"] == 0) and np.all(got["steps_done"] == K) and got["switches"].min() >= 0 and got["switches"].max() > 0
    for use_policy, out in ((True, got), (False, plain)):
        for b in range(B):
            for c in range(S):
                x, up, n_sw = x0[b], u_prev[b], 0
                for k in range(K):
                    u = policy.apply_np(P, midx[b:b + 1], x[None], up[None], u_seq[b, k][None])[0] if use_policy else u_seq[b, k]
                    if use_policy:
                        assert u[2] == u_seq[b, k, 2]
                        n_sw += int((u[:2] != up[:2]).sum())
                    aux = fn(x[None], u[None], om_seq[b, c, k][None], midx[b:b + 1])["v"][0]
                    one = models[midx[b]].lsim_k(x_k=x, v_k=np.concatenate([u, aux]), omega_k=om_seq[b, c, k])
                    assert np.array_equal(out["x"][b, c, k], x) and np.array_equal(out["v"][b, c, k], one["v"][:, 0]), (use_policy, b, c, k)
                    assert np.array_equal(out["x"][b, c, k + 1], one["x_k1"][:, 0]) and np.array_equal(out["y"][b, c, k], one["y"][:, 0]), (use_policy, b, c, k)
                    x, up = one["x_k1"][:, 0], u
                if use_policy:
                    assert out["switches"][b, c] == n_sw, (b, c)
    # u_prev=None: the policy's reset state
    reset = simlog.rollout_np(mats_list, d, midx, x0, u_seq, om_seq, fn, policy=P)
    again = simlog.rollout_np(mats_list, d, midx, x0, u_seq, om_seq, fn, policy=P, u_prev=P.initial_state(midx))
    for k in got:
        assert np.array_equal(reset[k], again[k], equal_nan=True), k


def test_threshold_controller_equals_the_loop():
    """the model without auxiliaries (lsim_k needs no resolver, so no device): feedback over three steps against apply_np + lsim_k; the first step has no
    previous record, so a tank inside the band stays off; the later ones read u_{k-1} from the log"""
    mats_list, models, d, midx, x0, om = _two_models(2, 3, hard=True, tie=False)
    assert d["ndelta"] == d["nz"] == d["nmu"] == 0
    m, nw = models[1], d["nomega"]
    P = policy.ThresholdPolicy.thermostat([58.5, 61.5, 63.5], [61.5, 63.5, 66.5], 2)
    x = np.array([57.0, 62.0, 65.0])                        # below its band: on; inside: off (no previous record); inside: off
    ctl = ThresholdController(m, P, x_k=x, omega_tilde_k=om[1], N_tilde=3, model_index=1)
    assert ctl.build() is None and not ctl.build_required
    up = P.initial_state(midx[1:2])[0]
    assert np.array_equal(up, np.zeros(3))
    seen = []
    for k in range(3):
        w = om[1].reshape(3, nw)[k]
        fb = ctl.feedback(k, omega_tilde_k=np.tile(w, 3))
        u = policy.apply_np(P, midx[1:2], x[None], up[None])[0]
        one = m.lsim_k(x_k=x, u_k=u, omega_k=w)
        assert np.array_equal(fb["u"][:, 0], u) and np.array_equal(fb["y"], one["y"]) and np.array_equal(fb["x"][:, 0], x) and "x_k1" not in fb, k
        sim = ctl.sim_step_k(k)
        assert np.array_equal(sim["x_k1"], one["x_k1"]) and np.array_equal(ctl.x_k, one["x_k1"]) and np.array_equal(ctl.sim_log[k]["u"][:, 0], u), k
        seen.append(u)
        x, up = one["x_k1"][:, 0], u
        if k == 0:
            assert np.array_equal(u, [1.0, 0.0, 0.0])
            ctl.x_k = x = np.array([60.0, 59.0, 70.0])      # tank 0 inside its band, on before: holds; tank 1 below: on; tank 2 above: off
    assert np.array_equal(seen[1], [1.0, 1.0, 0.0])
