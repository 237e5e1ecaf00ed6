"""The open-loop rollout (mld_rollout_batch / GpuProblem.rollout, kernel k_rollout) at the boundary of the library and in numpy, without a GPU: the header
and the binding agree on the new entry point, the options struct kept its size, the entry point follows the conventions of the others, and
simlog.rollout_np -- the reference of the device tests -- equals a loop over the package's MldModel.lsim_k with the closed form of tests/_aux_ref.py."""
import ctypes as C
import os
import re

import numpy as np

import _rollout_ref
import pyhybridcontrol_amd as phc
from pyhybridcontrol_amd import _lib, simlog, synthetic as syn

HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mldgpu.h")).read()


def test_header_and_binding_agree_on_the_entry_point():
    proto = (r"int\s+mld_rollout_batch\s*\(\s*mld_problem_t\s*\*\s*p\s*,\s*mld_problem_t\s*\*\s*aux\s*,\s*int\s+K\s*,\s*int\s+S\s*,\s*const\s+double\s*\*\s*u_seq\s*,"
             r"\s*const\s+double\s*\*\s*omega_seq\s*,\s*const\s+int64_t\s*\*\s*start\s*,\s*int\s+step\s*,\s*const\s+double\s*\*\s*cost_w\s*,\s*int\s+cost_rows\s*,"
             r"\s*double\s*\*\s*x_out\s*,\s*double\s*\*\s*v_out\s*,\s*double\s*\*\s*y_out\s*,\s*double\s*\*\s*cons_vio_out\s*,\s*int32_t\s*\*\s*cons_row_out\s*,"
             r"\s*double\s*\*\s*cost_out\s*,\s*double\s*\*\s*mu_total_out\s*,\s*double\s*\*\s*worst_vio_out\s*,\s*int32_t\s*\*\s*worst_step_out\s*,"
             r"\s*int32_t\s*\*\s*steps_done_out\s*,\s*int32_t\s*\*\s*end_status_out\s*,\s*int64_t\s+stats\[4\]\s*\)\s*;")
    assert re.search(proto, HDR)
    assert "mld_model.py:543-642" in HDR and ":701-766" in HDR                        # declared with the reference lines it replaces
    assert "mld_rollout_batch" in _lib.EXPORTS and hasattr(_lib.load(), "mld_rollout_batch")
    assert len(_lib.load().mld_rollout_batch.argtypes) == 22


def test_opts_size_is_unchanged():
    assert int(_lib.load().mld_opts_size()) == C.sizeof(_lib.Opts) == 64


def test_entry_point_without_a_device_or_a_handle():
    lib = _lib.load()
    x, es, stats = np.full(8, 7.0), np.full(2, 7, np.int32), np.full(4, 7, np.int64)
    rc = lib.mld_rollout_batch(None, None, 2, 1, None, None, None, 0, None, 0, _lib.dptr(x), None, None, None, None, None, None, None, None, None,
                               es.ctypes.data_as(C.POINTER(C.c_int32)), stats.ctypes.data_as(C.POINTER(C.c_int64)))
    if _lib.device_count() < 1:
        assert rc == -2 and b"no HIP device" in lib.mld_last_error()                  # MLD_ERR_NO_DEVICE, before anything else
    else:
        assert rc == -1 and b"no batch resident" in lib.mld_last_error()              # MLD_ERR_INVALID: no handle
    assert np.all(x == 7.0) and np.all(es == 7) and np.all(stats == 7)


def test_rollout_np_equals_a_loop_over_lsim_k():
    """make_agent(3) x 2 models, 4 instances x 3 realisations x 5 steps; the closed form re-derives delta, z, mu at every step.  Every field is equal."""
    B, S, K, N = 4, 3, 5, 3
    mats_list, models, xs, oms = [], [], [], []
    for k in range(2):
        rng = np.random.default_rng(8800 + k)
        mats, d, _ = syn.make_agent(3, rng, tie=True)
        x0, om = syn.make_scenarios(3, N, B, rng, tie=True)
        mats_list.append(mats); xs.append(x0); oms.append(om)
        models.append(phc.MldModel(nu_l=d["nu_l"], **mats))
    midx = np.arange(B) % 2
    x0, om = np.stack(xs)[midx, np.arange(B)], np.stack(oms)[midx, np.arange(B)]
    x0[1, 0], x0[2, 2] = 47.0, 80.5                                                   # slack on both sides
    rng = np.random.default_rng(8810)
    u_seq = (rng.uniform(size=(B, K, d["nu"])) < 0.4).astype(float)
    _, _, _, om_seq = _rollout_ref.realised_library(om, N, d["nomega"], d["nx"], S, K, 1, rng)
    assert np.all(np.abs(_rollout_ref.closed_y(mats_list, d, midx, u_seq, om_seq)) >= 1e-3)
    fn = _rollout_ref.closed_form_resolver(mats_list, d)
    cw = rng.uniform(0.5, 2.0, size=(B, K, 2 + d["nu"] + d["nmu"]))
    got = simlog.rollout_np(mats_list, d, midx, x0, u_seq, om_seq, fn, cost_w=cw)
    assert np.all(got["end_status"] == 0) and np.all(got["steps_done"] == K)
    assert (got["v"][..., d["nu"]] == 0).any() and (got["v"][..., d["nu"]] == 1).any() and (got["v"][..., d["nu"] + 2:] > 0).any()
    for b in range(B):
        for c in range(S):
            x = x0[b]
            cost = mu = 0.0
            vio = []
            for k in range(K):
                aux = fn(x[None], u_seq[b, k][None], om_seq[b, c, k][None], midx[b:b + 1])["v"][0]
                v = np.concatenate([u_seq[b, k], aux])
                one = models[midx[b]].lsim_k(x_k=x, v_k=v, omega_k=om_seq[b, c, k])
                assert np.array_equal(got["x"][b, c, k], x) and np.array_equal(got["v"][b, c, k], one["v"][:, 0]), (b, c, k)
                assert np.array_equal(got["x"][b, c, k + 1], one["x_k1"][:, 0]) and np.array_equal(got["y"][b, c, k], one["y"][:, 0]), (b, c, k)
                assert bool(np.all(one["cons"])) == bool(got["cons_vio"][b, c, k] <= simlog.CONS_TOL), (b, c, k)
                ref = simlog.lsim_k_batch([mats_list[midx[b]]], d, None, x[None], v[None], om_seq[b, c, k][None])
                row = got["cons_row"][b, c, k]                                        # (the kernels' order of the same sums differs by rounding only)
                assert abs(got["cons_vio"][b, c, k] - ref["resid"][0, row]) <= simlog.sum_bound(d) * ref["terms_r"][0, row], (b, c, k)
                assert ref["resid"][0, row] >= ref["cons_vio"][0] - 2 * simlog.sum_bound(d) * ref["terms_r"][0].max(), (b, c, k)
                vio.append(got["cons_vio"][b, c, k])
                cost += float(cw[b, k] @ v); mu += float(aux[2:].sum())
                x = one["x_k1"][:, 0]
            assert abs(got["cost"][b, c] - cost) <= 1e-12 * abs(cost) and abs(got["mu_total"][b, c] - mu) <= 1e-12 * max(1.0, mu), (b, c)
            assert got["worst_vio"][b, c] == max(vio) and got["worst_step"][b, c] == int(np.argmax(vio)), (b, c)
