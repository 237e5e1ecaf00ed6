"""CPU tests of the rollout risk (simlog.RiskTable, simlog.rollout_risk_np; mld_rollout_risk / GpuProblem.rollout(risk=...)): the numpy rule against an
independent restatement -- Python's sorted on (value, c) and a recursive tree sum --, the rank table, ties, mixed endings, the ABI, the wrapper's signature
and the stand-alone host check of k_rollout_risk's per-instance core under the address and undefined-behaviour sanitizers.  No GPU needed."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _aux_ref
import _rollout_ref
from test_rollout_kpi_host import B, K, N, S, _table, _trajectories
from pyhybridcontrol_amd import _lib, gpu, simlog, synthetic as syn
from pyhybridcontrol_amd.simlog import KpiTable, RiskTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (0.25, 0.5, 0.75, 1.0, 1.0 / 3.0, 1e-9, 0.9)
FLOATS = ("mean", "min", "max", "quantile", "cvar_hi", "cvar_lo")
INTS = ("min_c", "max_c", "n_exceed", "quantile_c") + simlog.RISK_COUNTS


def _with_kpis(d, midx, om_seq, traj, seed=8900):
    """the dict rollout(kpis=...) returns, from the numpy rollout: the summaries and "kpi"; the table has the input channel's selector u_0"""
    t = _table(d, np.random.default_rng(seed))
    price = np.random.default_rng(seed + 1).uniform(0.5, 2.0, (B, K, 2))
    out = dict(traj)
    out["kpi"] = simlog.rollout_kpis_np(traj, t, price=price, omega_seq=om_seq, model_idx=midx)
    return t, out


def _columns(kpis, level=0.0):
    r = RiskTable(kpis, LEVELS)
    r.add("cost", "cost").add("mu", "mu_total", level=level).add("vio", "worst_vio", level=1e-6).add("n_vio", "n_vio", level=0.0)
    for src in ("kpi_sum", "kpi_min", "kpi_max", "kpi_n_above", "kpi_n_changes"):
        for name in ("x_only", "all_five", "u_0"):
            r.add("%s:%s" % (src, name), src, kpi=name, level=level)
    return r


def _tree(leaves):
    if len(leaves) == 1:
        return leaves[0]
    h = len(leaves) // 2
    return np.float64(_tree(leaves[:h])) + np.float64(_tree(leaves[h:]))


def _restated(out, risk, policy=False):
    """the rule once more, one (instance, column) at a time, in plain Python"""
    arr = risk.arrays()
    es = np.asarray(out["end_status"])
    nB, nS = es.shape
    G, L = len(risk), len(risk.levels)
    level = np.full(G, np.inf) if arr["level"] is None else arr["level"]
    res = {k: np.zeros((nB, G) + ((L,) if k in simlog.RISK_LEVEL_KEYS else ())) for k in simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS}
    res.update({k: np.zeros(nB) for k in simlog.RISK_COUNTS})
    kk = {5: "sum", 6: "min", 7: "max", 8: "n_above", 9: "n_changes"}
    for b in range(nB):
        for key, e in zip(simlog.RISK_COUNTS, (0, 1, 2, -1)):
            res[key][b] = sum(1 for c in range(nS) if es[b, c] == e)
        done = [c for c in range(nS) if es[b, c] == 0]
        n = len(done)
        for j in range(G):
            src, q = int(arr["col_src"][j]), int(arr["col_q"][j])
            col = out[simlog.RISK_SOURCES[src]][b] if src < 4 else out["kpi"]["n_vio"][b] if src == 4 else out["kpi"][kk[src]][b, :, q]
            g = [np.float64(col[c]) for c in range(nS)]
            order = sorted(done, key=lambda c: (math.isnan(g[c]), 0.0 if math.isnan(g[c]) else g[c], c))
            leaf = lambda pick: [g[c] if pick(c) else np.float64(0.0) for c in range(nS)] + [np.float64(0.0)] * (64 - nS)
            res["mean"][b, j] = _tree(leaf(lambda c: c in done)) / np.float64(n) if n else np.nan
            lo, lo_c, hi, hi_c = np.inf, -1, -np.inf, -1
            for c in done:
                if g[c] < lo:
                    lo, lo_c = g[c], c
                if g[c] > hi:
                    hi, hi_c = g[c], c
            res["min"][b, j], res["min_c"][b, j], res["max"][b, j], res["max_c"][b, j] = lo, lo_c, hi, hi_c
            res["n_exceed"][b, j] = sum(1 for c in done if g[c] > level[j])
            for l, a in enumerate(risk.levels):
                if not n:
                    res["quantile"][b, j, l] = res["cvar_hi"][b, j, l] = res["cvar_lo"][b, j, l] = np.nan
                    res["quantile_c"][b, j, l] = -1
                    continue
                i = 0
                while not (float(i + 1) >= a * float(n)):
                    i += 1
                srt = [g[c] for c in order] + [np.float64(0.0)] * (64 - n)
                res["quantile"][b, j, l], res["quantile_c"][b, j, l] = srt[i], order[i]
                res["cvar_hi"][b, j, l] = _tree([srt[r] if i <= r < n else np.float64(0.0) for r in range(64)]) / np.float64(n - i)
                res["cvar_lo"][b, j, l] = _tree([srt[r] if r <= i else np.float64(0.0) for r in range(64)]) / np.float64(i + 1)
    return res


def _same(got, want, what):
    for k in FLOATS:
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        ok = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        assert a.shape == b.shape and np.all(ok), (what, k, a[~ok][:4], b[~ok][:4])
    for k in INTS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], np.asarray(want[k]).astype(np.int32)), (what, k)


def test_numpy_rule_against_the_restatement_and_np_quantile():
    d, midx, om_seq, traj = _trajectories()
    kpis, out = _with_kpis(d, midx, om_seq, traj)
    risk = _columns(kpis, level=float(np.median(out["mu_total"])))
    got = simlog.rollout_risk_np(out, risk)
    assert got["names"] == risk.names and got["levels"] == list(LEVELS)
    assert got["mean"].shape == (B, len(risk)) and got["quantile"].shape == (B, len(risk), len(LEVELS)) and got["n_complete"].shape == (B,)
    assert np.all(got["n_complete"] == S)
    _same(got, _restated(out, risk), "complete")
    assert (got["n_exceed"] > 0).any() and (got["n_exceed"] < S).any()
    # dyadic levels: the quantile is numpy's inverted CDF
    arr = risk.arrays()
    kk = {5: "sum", 6: "min", 7: "max", 8: "n_above", 9: "n_changes"}
    for j in range(len(risk)):
        src, q = int(arr["col_src"][j]), int(arr["col_q"][j])
        col = out[simlog.RISK_SOURCES[src]] if src < 4 else out["kpi"]["n_vio"] if src == 4 else out["kpi"][kk[src]][:, :, q]
        for l, a in enumerate(LEVELS[:4]):
            assert np.array_equal(got["quantile"][:, j, l], np.quantile(np.asarray(col, np.float64), a, axis=1, method="inverted_cdf")), (j, a)
    # alpha = 1: the upper tail is the maximum, the lower tail the tree mean of everything
    one = LEVELS.index(1.0)
    assert np.array_equal(got["quantile"][:, :, one], got["max"]) and np.array_equal(got["cvar_hi"][:, :, one], got["max"])
    scale = 4.0 * 2.0 ** -52 * np.maximum(np.abs(got["min"]), np.abs(got["max"]))      # S = 3 terms in another order: two roundings either way
    assert np.all(np.abs(got["cvar_lo"][:, :, one] - got["mean"]) <= scale)
    tiny = LEVELS.index(1e-9)
    assert np.array_equal(got["quantile"][:, :, tiny], got["min"]) and np.array_equal(got["cvar_lo"][:, :, tiny], got["min"])
    assert np.all(np.abs(got["cvar_hi"][:, :, tiny] - got["mean"]) <= scale)
    # a policy's switch counts, NaN values and both zeros through the same restatement
    rng = np.random.default_rng(8910)
    odd = dict(out, switches=rng.integers(0, 3, (B, S)).astype(np.int32), cost=np.array([[0.0, -0.0, 0.0], [np.nan, 1.0, np.nan], [-0.0, np.nan, 0.0], [np.nan] * 3]))
    r2 = RiskTable(None, LEVELS).add("sw", "switches", level=1.0).add("cost", "cost", level=-1.0)
    g2 = simlog.rollout_risk_np(odd, r2, policy=True)
    _same(g2, _restated(odd, r2), "switches, NaN, zeros")
    assert list(g2["min_c"][:, 1]) == [0, 1, 0, -1] and list(g2["max_c"][:, 1]) == [0, 1, 0, -1] and list(g2["quantile_c"][1, 1, :4]) == [1, 0, 2, 2]
    assert np.signbit(g2["max"][2, 1]) and not np.signbit(g2["max"][0, 1])      # the value at the winning c: -0.0 at c = 0 of instance 2
    with pytest.raises(ValueError, match="policy"):
        simlog.rollout_risk_np(odd, r2)


def test_rank_table():
    for n in range(1, 65):
        idx = simlog.risk_rank_table([1.0 / n, 1.0, 1e-9], 64)
        assert idx.shape == (3, 64) and idx.dtype == np.int32
        assert idx[0, n - 1] == 0 and idx[2, n - 1] == 0 and idx[1, n - 1] == n - 1
    idx = simlog.risk_rank_table([0.5, 0.95], 20)
    assert list(idx[0, :6]) == [0, 0, 1, 1, 2, 2] and idx[1, 19] == 18 and idx[1, 18] == 18 and idx[0, 19] == 9
    for a in (0.05, 0.3, 0.7, 0.999):      # ceil(alpha n) - 1 wherever the product is not within a rounding of an integer
        idx = simlog.risk_rank_table([a], 64)[0]
        for n in range(1, 65):
            if abs(a * n - round(a * n)) > 1e-9:
                assert idx[n - 1] == math.ceil(a * n) - 1, (a, n)


def test_ties_take_the_smallest_realisation():
    """open loop: every realisation of an instance applies the same u_seq, so the input channel's n_changes is the same over c"""
    d, midx, om_seq, traj = _trajectories()
    kpis, out = _with_kpis(d, midx, om_seq, traj)
    chg = out["kpi"]["n_changes"][:, :, kpis.names.index("u_0")]
    assert np.all(chg == chg[:, :1]) and chg.max() > 0      # the tie is there
    risk = RiskTable(kpis, LEVELS).add("switching", "kpi_n_changes", kpi="u_0")
    got = simlog.rollout_risk_np(out, risk)
    assert np.all(got["min_c"] == 0) and np.all(got["max_c"] == 0)
    idx = simlog.risk_rank_table(LEVELS, S)[:, S - 1]
    assert np.array_equal(got["quantile_c"][:, 0, :], np.broadcast_to(idx, (B, len(LEVELS))))      # sorted by c alone: rank i is realisation i
    assert np.array_equal(got["quantile"][:, 0, :], np.broadcast_to(chg[:, :1].astype(float), (B, len(LEVELS))))
    assert np.array_equal(got["mean"][:, 0], chg[:, 0].astype(float)) and np.array_equal(got["min"], got["max"])
    _same(got, _restated(out, risk), "ties")


def _mixed():
    """the hard variant of _trajectories' scenario (x0 as drawn) with realisation 1's disturbance scaled by 5"""
    mats_list, xs, oms = [], [], []
    for k in range(2):
        rng = np.random.default_rng(8800 + k)
        mats, d, _ = syn.make_agent(3, rng, tie=True)
        mats, d = _aux_ref.hard_variant(mats, d)
        x0, om = syn.make_scenarios(3, N, B, rng, tie=True)
        mats_list.append(mats); xs.append(x0); oms.append(om)
    midx = np.arange(B) % 2
    x0, om = np.stack(xs)[midx, np.arange(B)], np.stack(oms)[midx, np.arange(B)]
    rng = np.random.default_rng(8810)
    u_seq = (rng.uniform(size=(B, K, d["nu"])) < 0.4).astype(float)
    _, _, _, om_seq = _rollout_ref.realised_library(om, N, d["nomega"], d["nx"], S, K, 1, rng)
    om_seq = np.array(om_seq)
    om_seq[:, 1] *= 5.0
    traj = simlog.rollout_np(mats_list, d, midx, x0, u_seq, om_seq, _rollout_ref.closed_form_resolver(mats_list, d))
    return d, midx, om_seq, traj


def test_mixed_endings():
    d, midx, om_seq, traj = _mixed()
    assert traj["end_status"].tolist() == [[0, 0, 0], [0, 1, 0], [1, 1, 1], [1, 1, 1]]
    kpis, out = _with_kpis(d, midx, om_seq, traj)
    risk = _columns(kpis)
    got = simlog.rollout_risk_np(out, risk)
    assert list(got["n_complete"]) == [3, 2, 0, 0] and list(got["n_infeasible"]) == [0, 1, 3, 3]
    assert not got["n_declined"].any() and not got["n_not_attempted"].any()
    _same(got, _restated(out, risk), "mixed endings")
    # instance 1: realisations 0 and 2 only
    j = risk.names.index("mu")
    mu = out["mu_total"][1]
    assert got["mean"][1, j] == (mu[0] + mu[2]) / 2.0 and got["min"][1, j] == min(mu[0], mu[2]) and got["max"][1, j] == max(mu[0], mu[2])
    assert np.all(np.isin(got["min_c"][1], (0, 2))) and np.all(np.isin(got["max_c"][1], (0, 2))) and np.all(np.isin(got["quantile_c"][1], (0, 2)))
    assert np.all(np.isfinite(got["mean"][:2])) and np.all(np.isfinite(got["quantile"][:2]))
    # the empty instances
    for k in ("mean", "quantile", "cvar_hi", "cvar_lo"):
        assert np.all(np.isnan(got[k][2:])), k
    assert np.all(got["min"][2:] == np.inf) and np.all(got["max"][2:] == -np.inf) and np.all(got["n_exceed"][2:] == 0)
    assert np.all(got["min_c"][2:] == -1) and np.all(got["max_c"][2:] == -1) and np.all(got["quantile_c"][2:] == -1)


def test_risk_table_checks():
    d, midx, om_seq, traj = _trajectories()
    kpis = _table(d, np.random.default_rng(1))
    r = RiskTable(kpis, (0.5,)).add("a", "cost")
    for kw, word in ((dict(name="a", source="cost"), "already"), (dict(name="b", source="nope"), "source"), (dict(name="b", source="kpi_sum", kpi="zz"), "not a KPI"),
                     (dict(name="b", source="cost", kpi="x_only"), "kpi given"), (dict(name="b", source="cost", level=np.nan), "NaN")):
        with pytest.raises(ValueError, match=word):
            r.add(**kw)
    with pytest.raises(ValueError, match="KPI table"):
        RiskTable().add("b", "n_vio")
    for bad in ((0.0,), (1.5,), (np.nan,), (0.5,) * 9):
        with pytest.raises(ValueError):
            RiskTable(None, bad)
    with pytest.raises(ValueError, match="no column"):
        RiskTable().arrays()
    full = RiskTable()
    for k in range(64):
        full.add("c%d" % k, "cost")
    with pytest.raises(ValueError, match="at most 64"):
        full.add("c64", "cost")
    a = RiskTable(kpis, (0.5, 1.0)).add("a", "kpi_max", kpi="v_only", level=2.0).add("b", "mu_total").arrays()
    assert a["col_src"].tolist() == [7, 1] and a["col_q"].tolist() == [1, 0] and a["level"].tolist() == [2.0, np.inf] and a["alpha"].tolist() == [0.5, 1.0]
    assert RiskTable().add("b", "mu_total").arrays()["level"] is None


def test_abi_declares_and_binds_the_entry_point():
    assert "mld_rollout_risk" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "mldgpu.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint mld_rollout_risk\(mld_problem_t \*p, mld_problem_t \*aux, int policy, int K, int S,", header)
    assert re.search(r"int G, const int32_t \*col_src, const int32_t \*col_q, const double \*level, int L, const double \*alpha,", header)
    for name, val in (("MLD_RISK_COLS_MAX", 64), ("MLD_RISK_LEVELS_MAX", 8), ("MLD_RISK_S_MAX", 64)):
        assert re.search(r"#define %s %d\b" % (name, val), header), name
    assert (simlog.RISK_COLS_MAX, simlog.RISK_LEVELS_MAX, simlog.RISK_S_MAX) == (64, 8, 64)
    lib = _lib.load()
    assert hasattr(lib, "mld_rollout_risk") and len(lib.mld_rollout_kpi.argtypes) == 43 and len(lib.mld_rollout_risk.argtypes) == 60
    assert list(lib.mld_rollout_risk.argtypes[:43]) == list(lib.mld_rollout_kpi.argtypes)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    src, alpha = np.zeros(2, np.int32), np.array([0.5])
    mean, qc, counts, cost = np.full(2, 7.0), np.full(2, 7, np.int32), np.full(4, 7, np.int32), np.full(2, 7.0)
    rc = lib.mld_rollout_risk(None, None, 0, 2, 1, None, None, None, None, 0, None, 0, 0, None, None, None, None, None, None, None, 1e-6, None,
                              None, None, None, None, None, _lib.dptr(cost), None, None, None, None, None, None, None, None, None, None, None, None, None, None, None,
                              2, ip(src), None, None, 1, _lib.dptr(alpha), _lib.dptr(mean), None, None, None, None, None, None, ip(qc), None, None, ip(counts))
    if _lib.device_count() < 1:
        assert rc == -2 and b"no HIP device" in lib.mld_last_error()
    else:
        assert rc == -1 and b"mld_rollout_risk" in lib.mld_last_error() and b"no batch resident" in lib.mld_last_error()
    assert np.all(mean == 7.0) and np.all(qc == 7) and np.all(counts == 7) and np.all(cost == 7.0)


def test_wrapper_signature():
    sig = inspect.signature(gpu.GpuProblem.rollout)
    names = list(sig.parameters)
    assert names[names.index("vio_tol") + 1:] == ["risk", "per_trajectory"]
    assert sig.parameters["risk"].default is None and sig.parameters["per_trajectory"].default is True
    assert names[:14] == ["self", "resolve", "K", "u_seq", "omega_seq", "start", "step", "cost_w", "trajectories", "policy", "u_prev", "kpis", "price_start", "vio_tol"]


def test_host_check_is_clean_under_the_sanitizers(tmp_path):
    """scripts/rollout_risk_host_check.cpp, its own executable: risk_instance at S = 1, 2, 3, 63, 64 on buffers of exactly the length the core may use,
    all-tied columns, n = 0 and n = 1, under ASan and UBSan"""
    exe = str(tmp_path / "rollout_risk_host_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pyhybridcontrol_amd", "csrc"),
           os.path.join(ROOT, "scripts", "rollout_risk_host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert ran.returncode == 0 and "every figure as the naive restatement gives it" in ran.stdout, ran.stdout
