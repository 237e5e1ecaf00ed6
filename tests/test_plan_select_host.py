"""CPU tests of the plan selection (simlog.PlanSelector, simlog.select_plan_np; mld_rollout_select / GpuProblem.select_plan): the numpy rule against an
independent restatement -- a Python loop with min over (value, p) tuples --, NaN, both infinities, both zeros, nobody admissible and min_complete, the
selector's validation, the ABI, the wrapper's signature, the unchanged argtypes of the two older rollout entries, the entry guard, and the stand-alone host
check of k_plan_select's rule under the address and undefined-behaviour sanitizers.  No GPU needed."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from pyhybridcontrol_amd import _lib, gpu, simlog
from pyhybridcontrol_amd.simlog import PlanSelector, RiskTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (0.5, 1.0, 0.25)
B, P, G, S = 40, 7, 3, 5


def _table():
    return RiskTable(None, LEVELS).add("cost", "cost", level=0.0).add("mu", "mu_total").add("vio", "worst_vio", level=1e-6)


def _risk(seed, special):
    """a per-candidate risk dict with the shapes select_plan(per_candidate=True) returns; special: NaN, +-inf and +-0.0 among few distinct values"""
    rng = np.random.default_rng(seed)
    L = len(LEVELS)

    def draw(shape):
        if special:
            return rng.choice(np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1.0]), size=shape)
        return rng.integers(-4, 5, size=shape) / 4.0      # dyadic, many ties

    r = {k: draw((B, P, G)) for k in ("mean", "min", "max")}
    r.update({k: draw((B, P, G, L)) for k in ("quantile", "cvar_hi", "cvar_lo")})
    r["n_exceed"] = rng.integers(0, 3, size=(B, P, G)).astype(np.int32)
    r["n_complete"] = rng.integers(0, S + 1, size=(B, P)).astype(np.int32)
    return r


def _restated(risk, sel, min_complete):
    """the rule once more, one instance at a time: min over (value, p) tuples of the admissible candidates"""
    arr = sel.arrays()

    def value(b, p, col, kind, lvl):
        a = risk[simlog.SELECT_KINDS[kind]]
        return float(a[b, p, col, lvl]) if kind >= 4 else float(a[b, p, col])

    choice, score, n_adm, adm = [], [], [], []
    for b in range(B):
        keys, row = [], []
        for p in range(P):
            v = value(b, p, *arr["obj"])
            ok = int(risk["n_complete"][b, p]) >= min_complete and not math.isnan(v)
            for k in range(arr["n_cons"]):
                c = value(b, p, int(arr["cons_col"][k]), int(arr["cons_kind"][k]), int(arr["cons_level"][k]))
                ok = ok and not math.isnan(c) and c <= float(arr["cons_bound"][k])
            row.append(ok)
            if ok:
                keys.append((v, p))      # Python compares -0.0 == 0.0, so the tuple's second entry decides: the smaller p
        adm.append(row)
        n_adm.append(len(keys))
        best = min(keys) if keys else (float("nan"), -1)
        choice.append(best[1])
        score.append(best[0])
    return dict(choice=np.array(choice, np.int32), score=np.array(score), n_admissible=np.array(n_adm, np.int32), admissible=np.array(adm, bool))


def _same(got, want, what):
    for k in simlog.SELECT_KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype)
        ok = ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == "f" else a == b
        assert np.all(ok), (what, k, a[~ok][:4], b[~ok][:4])


def _selectors(t):
    for kind in simlog.SELECT_KINDS:
        lvl = dict(level=0.25) if kind in simlog.SELECT_KINDS[4:] else {}
        yield kind, 0, PlanSelector(t).minimise("mu", kind, **lvl)
        yield kind, 1, PlanSelector(t).minimise("cost", kind, **lvl).subject_to("vio", "max", 0.5)
        s = PlanSelector(t).minimise(2, kind, **lvl)
        for k in range(8):
            s.subject_to(k % 3, simlog.SELECT_KINDS[k % 7], (1.0, np.inf, 0.0)[k % 3], level=(k % 3 if k % 7 >= 4 else None))
        yield kind, 8, s


@pytest.mark.parametrize("special", [False, True])
def test_numpy_rule_against_the_restatement(special):
    t = _table()
    risk = _risk(9300 + special, special)
    seen = set()
    for kind, n_cons, sel in _selectors(t):
        for mc in (1, 3, S):
            got = simlog.select_plan_np(risk, sel, mc)
            _same(got, _restated(risk, sel, mc), (kind, n_cons, mc))
            seen |= {-1} & set(got["choice"].tolist()) | ({0} & set(got["choice"].tolist())) | ({1} if (got["choice"] >= 1).any() else set())
            assert np.all(np.isnan(got["score"]) == (got["choice"] < 0)) and np.all((got["n_admissible"] == 0) == (got["choice"] < 0))
    assert seen == {-1, 0, 1}      # no choice, the first candidate, a later one: all three occurred


def test_corners():
    t = RiskTable(None, ()).add("cost", "cost")
    sel = PlanSelector(t).minimise("cost", "mean")

    def risk(mean, n=None):
        mean = np.asarray(mean, dtype=np.float64)
        r = dict(mean=mean[:, :, None], n_complete=np.full(mean.shape, 2, np.int32) if n is None else np.asarray(n, np.int32))
        return r

    nan, inf = np.nan, np.inf
    got = simlog.select_plan_np(risk([[0.0, -0.0, 0.0], [-0.0, 0.0, 1.0], [nan, 2.0, 2.0], [nan, nan, nan], [inf, inf, -inf], [inf, nan, inf]]), sel, 1)
    assert got["choice"].tolist() == [0, 0, 1, -1, 2, 0] and got["n_admissible"].tolist() == [3, 3, 2, 0, 3, 2]
    assert not np.signbit(got["score"][0]) and np.signbit(got["score"][1]) and np.isnan(got["score"][3]) and got["score"][4] == -inf and got["score"][5] == inf
    # an inadmissible +inf in front of an admissible +inf
    got = simlog.select_plan_np(risk([[inf, inf, 3.0]], n=[[0, 2, 1]]), sel, 2)
    assert got["choice"].tolist() == [1] and got["admissible"].tolist() == [[False, True, False]] and got["score"][0] == inf
    # min_complete
    r = risk([[1.0, 2.0, 3.0]], n=[[1, 2, 3]])
    assert [simlog.select_plan_np(r, sel, mc)["choice"][0] for mc in (1, 2, 3)] == [0, 1, 2]
    # a bound is met with equality; a NaN constraint value fails
    con = PlanSelector(t).minimise("cost", "mean").subject_to("cost", "min", 1.0)
    r = dict(mean=np.array([[[0.0], [1.0], [2.0]]]), min=np.array([[[nan], [1.0], [1.5]]]), n_complete=np.full((1, 3), 2, np.int32))
    got = simlog.select_plan_np(r, con, 1)
    assert got["choice"].tolist() == [1] and got["admissible"].tolist() == [[False, True, False]]
    # the chosen inputs
    cand = np.arange(1 * 3 * 2 * 2, dtype=np.float64).reshape(1, 3, 2, 2)
    got = simlog.select_plan_np(r, con, 1, candidates=cand)
    assert np.array_equal(got["u"], cand[:, 1]) and np.array_equal(got["u0"], cand[:, 1, 0])
    got = simlog.select_plan_np(r, con, 3, candidates=cand)
    assert got["choice"].tolist() == [-1] and np.all(np.isnan(got["u"])) and np.all(np.isnan(got["u0"])) and got["u"].shape == (1, 2, 2)


def test_plan_selector_checks():
    t = _table()
    with pytest.raises(ValueError, match="RiskTable"):
        PlanSelector(None)
    with pytest.raises(ValueError, match="RiskTable"):
        PlanSelector(RiskTable())
    with pytest.raises(ValueError, match="no objective"):
        PlanSelector(t).arrays()
    for args, kw, word in ((("nope", "mean"), {}, "not a column"), ((3, "mean"), {}, "3 columns"), (("cost", "median"), {}, "kind"),
                           (("cost", "mean"), dict(level=0.5), "not per level"), (("cost", "quantile"), {}, "per level"),
                           (("cost", "cvar_hi"), dict(level=0.3), "not a level"), (("cost", "cvar_lo"), dict(level=3), "3 levels")):
        with pytest.raises(ValueError, match=word):
            PlanSelector(t).minimise(*args, **kw)
    s = PlanSelector(t).minimise("mu", "cvar_hi", level=1.0)
    with pytest.raises(ValueError, match="already"):
        s.minimise("mu", "mean")
    with pytest.raises(ValueError, match="NaN"):
        s.subject_to("vio", "max", np.nan)
    for k in range(8):
        s.subject_to("vio", "quantile", float(k), level=2)
    with pytest.raises(ValueError, match="at most 8"):
        s.subject_to("vio", "max", 0.0)
    a = s.arrays()
    assert a["obj"] == (1, 5, 1) and a["n_cons"] == 8 and a["cons_col"].tolist() == [2] * 8 and a["cons_kind"].tolist() == [4] * 8
    assert a["cons_level"].tolist() == [2] * 8 and a["cons_bound"].tolist() == [float(k) for k in range(8)] and a["cons_col"].dtype == np.int32
    assert PlanSelector(t).minimise(0, "n_exceed").arrays()["obj"] == (0, 3, 0)
    assert (simlog.SELECT_P_MAX, simlog.SELECT_CONS_MAX) == (64, 8)


def test_abi_declares_and_binds_the_entry_point():
    assert "mld_rollout_select" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "mldgpu.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint mld_rollout_select\(mld_problem_t \*p, mld_problem_t \*aux, int K, int S, int P, int plan_first, const double \*u_cand,", header)
    assert re.search(r"int obj_col, int obj_kind, int obj_level, int n_cons, const int32_t \*cons_col, const int32_t \*cons_kind, const int32_t \*cons_level,", header)
    for name, val in (("MLD_SELECT_P_MAX", 64), ("MLD_SELECT_CONS_MAX", 8)):
        assert re.search(r"#define %s %d\b" % (name, val), header), name
    lib = _lib.load()
    assert hasattr(lib, "mld_rollout_select") and len(lib.mld_rollout_select.argtypes) == 69
    # the two older rollout entries are bound as they were
    assert len(lib.mld_rollout_kpi.argtypes) == 43 and len(lib.mld_rollout_risk.argtypes) == 60
    assert list(lib.mld_rollout_risk.argtypes[:43]) == list(lib.mld_rollout_kpi.argtypes)
    # the entry guard on a NULL handle: refused, nothing written
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    src, alpha = np.zeros(1, np.int32), np.array([0.5])
    choice, score, u0 = np.full(2, 7, np.int32), np.full(2, 7.0), np.full(2, 7.0)
    args = [None, None, 2, 1, 1, 1, None, None, None, 0, None, 0, 0, None, None, None, None, None, None, None, 1e-6, None,
            1, ip(src), None, None, 1, _lib.dptr(alpha), 0, 0, 0, 0, None, None, None, None, 1,
            ip(choice), _lib.dptr(score), None, None, None, _lib.dptr(u0)] + [None] * 26
    assert len(args) == 69
    rc = lib.mld_rollout_select(*args)
    if _lib.device_count() < 1:
        assert rc == -2 and b"no HIP device" in lib.mld_last_error()
    else:
        assert rc == -1 and b"mld_rollout_select" in lib.mld_last_error() and b"no batch resident" in lib.mld_last_error()
    assert np.all(choice == 7) and np.all(score == 7.0) and np.all(u0 == 7.0)


def test_wrapper_signature():
    sig = inspect.signature(gpu.GpuProblem.select_plan)
    assert list(sig.parameters) == ["self", "resolve", "selector", "candidates", "plan_first", "K", "omega_seq", "start", "step", "cost_w", "kpis", "price_start",
                                    "vio_tol", "min_complete", "per_candidate", "per_trajectory"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["candidates"] is None and d["plan_first"] is False and d["K"] is None and d["step"] == 0 and d["vio_tol"] == 1e-6 and d["min_complete"] is None
    assert d["per_candidate"] is False and d["per_trajectory"] is False
    assert list(inspect.signature(simlog.select_plan_np).parameters)[:3] == ["risk_per_candidate", "selector", "min_complete"]
    # rollout() is what it was
    names = list(inspect.signature(gpu.GpuProblem.rollout).parameters)
    assert names == ["self", "resolve", "K", "u_seq", "omega_seq", "start", "step", "cost_w", "trajectories", "policy", "u_prev", "kpis", "price_start", "vio_tol",
                     "risk", "per_trajectory"]


def test_host_check_is_clean_under_the_sanitizers(tmp_path):
    """scripts/plan_select_host_check.cpp, its own executable: the rule's functions, the serial scan and a simulated butterfly for P = 1 .. 64 on arrays of
    exactly the length the rule may read, random, tied and special values, under ASan and UBSan"""
    exe = str(tmp_path / "plan_select_host_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pyhybridcontrol_amd", "csrc"),
           os.path.join(ROOT, "scripts", "plan_select_host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert ran.returncode == 0 and "every choice as the naive restatement gives it" in ran.stdout, ran.stdout
