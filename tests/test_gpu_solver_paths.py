"""Every version of k_solve's pivot loop and cut builders against HiGHS.

A. Placement.  build_shape puts each hot per-basis array in LDS while it fits its budget and leaves it in the slot otherwise; the offsets pick the
   code: the typed all-LDS pivot loop (s_dual_simplex_impl<true>) or the generic one, the reduced-cost row in LDS or behind the dictionary, the
   c-MIR scoring lines compact in LDS / full width in LDS / in the slot, and with them a wave per cut or block-wide c-MIR phase B.  MLD_SOL_SLOT
   keeps the named arrays in the slot; GpuProblem.debug_shape() shows where each one went, and every case asserts it reached its placement.
B. The diagnostic switches of mld_opts.reserved (mld_reserved_bit): each must still prove the HiGHS optimum.  Deliberately excluded: bit 0
   (solver trace: builds with -DMLD_TRACE only) and bit 20 (positive control of the assertion build: it exists to make an index check fail).
C. Cut-row capacity and dictionary shape edges: unpadded rows (ld == n + 1), fewer rows than waves, more rows than threads, cut rows that fill
   during the first round, no cut rows, one cut per round, no / one rounding cut per round.

Workloads: W1 = cfg2 (100 binaries, n = 275, m0 = 300), W2 = six random non-tank models (tests/_paths.fuzz_mld), W3 = the cfg2 MIQP.  The
references are HiGHS (scipy.optimize.milp, mip_rel_gap = 0) on the ORIGINAL rows for W1 / W2 and the C oracle's MIQP for W3, computed once per
module.
"""
import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

import condense_np as cn
import orc
import tighten_np
from _paths import fuzz_mld
from pyhybridcontrol_amd import MldGpuError, gpu, host, synthetic as syn

pytestmark = pytest.mark.gpu

HOT = ("lXB", "lBasic", "lSkip", "lAtUp", "lNonbasic", "lXN", "lLo", "lHi", "lDw", "lCost")
SLOT_FIELDS = dict(xb=("lXB",), basic=("lBasic",), skip=("lSkip",), atup=("lAtUp",), nonbasic=("lNonbasic",), xn=("lXN",), lohi=("lLo", "lHi"),
                   dw=("lDw",), cost=("lCost",), mirline=("lMirLine",), mircache=("lMirCache",))
W2_SEEDS = (0, 1, 2, 5, 7, 11)
W2_BATCH = 6
MIR_SERIAL, NO_RESTART, LAZY_START, NO_SWEEP = 1 << 15, 1 << 16, 1 << 17, 1 << 19
EXACT = dict(max_nodes=50000, max_pivots=400000)


class Work(object):
    """one model, its instances and the HiGHS answers on its original rows"""

    def __init__(self, name, mats, dims, atoms, N_p, N, x0, om, quadratic=False):
        self.name, self.mats, self.dims, self.atoms, self.N_p, self.N, self.x0, self.om = name, mats, dims, atoms, N_p, N, x0, om
        self.batch = x0.shape[0]
        self.cost = host.cost_from_atoms(atoms, dims, N_p, N)
        self.model = gpu.GpuModel([mats], dims)
        self.raw = cn.standard_form(mats, atoms, N_p, N, nu_l=dims["nu_l"])
        self.isb = self.raw["is_bin"].astype(bool)
        self.rown = np.maximum(1.0, np.abs(self.raw["G"]).max(axis=1))
        self.h = np.stack([cn.rhs(self.raw["evo"], x0[s], self._w(s)) for s in range(self.batch)])
        self.r = np.array([cn.cost_const(self.raw["cost"]["const_terms"], x0[s], self._w(s)) for s in range(self.batch)])
        self.ref = np.full(self.batch, np.nan)
        self.unbounded = np.zeros(self.batch, bool)
        self.quadratic = quadratic
        if quadratic:           # like tests/test_gpu_miqp.py: the C oracle's MIQP on the tightened rows
            sft = cn.standard_form(tighten_np.tighten(mats, dims, nu_l=dims["nu_l"]), atoms, N_p, N, nu_l=dims["nu_l"])
            for s in range(self.batch):
                q, r = cn.lin_cost(sft["cost"], x0[s], self._w(s)), cn.cost_const(sft["cost"]["const_terms"], x0[s], self._w(s))
                o = orc.solve_miqp(sft["cost"]["P"], q, sft["G"], cn.rhs(sft["evo"], x0[s], self._w(s)), sft["lb"], sft["ub"], sft["is_bin"],
                                   max_nodes=20000, presolve=0, gap_rel=1e-6)
                assert o["status"] == "optimal", (name, s, o["status"])
                self.ref[s] = o["obj"] + r
            return
        for s in range(self.batch):
            q = cn.lin_cost(self.raw["cost"], x0[s], self._w(s))
            res = milp(q, constraints=LinearConstraint(self.raw["G"], -np.inf, self.h[s]), integrality=self.raw["is_bin"].astype(int),
                       bounds=Bounds(self.raw["lb"], self.raw["ub"]), options=dict(mip_rel_gap=0.0))
            if res.status == 3:
                self.unbounded[s] = True
                continue
            assert res.status == 0, (name, s, res.status)
            self.ref[s] = res.fun + self.r[s]

    def _w(self, s):
        return self.om[s] if self.dims["nomega"] else np.zeros(0)

    def problem(self, **opts):
        return gpu.GpuProblem(self.model, self.N_p, self.N, self.cost, **opts)

    def solve(self, p, warm_start=None):
        return p.solve(self.x0, self.om, warm_start=warm_start)

    def value(self, v, s):
        q = cn.lin_cost(self.raw["cost"], self.x0[s], self._w(s))
        val = q @ v + self.r[s]
        if self.quadratic:
            val += 0.5 * v @ self.raw["cost"]["P"] @ v
        return val

    def check(self, out, what, gap=0.0):
        """status optimal (unbounded exactly where HiGHS says so); objective at the reference (within `gap` relative above it when the solve
        ran with a gap); lower bound not above it; binaries exactly 0 / 1; the point feasible for the original rows and worth its objective"""
        tol_obj = 2e-6 if self.quadratic else 1e-6         # (W3: the oracle's own gap is 1e-6, as in tests/test_gpu_miqp.py)
        for s in range(self.batch):
            tag = (self.name, what, s)
            if self.unbounded[s]:
                assert out["status"][s] == 4, tag + (int(out["status"][s]),)
                continue
            ref, sc = self.ref[s], max(1.0, abs(self.ref[s]))
            assert out["status"][s] == 0, tag + (int(out["status"][s]), int(out["nodes"][s]))
            if gap > 0.0:
                assert ref - tol_obj * sc <= out["obj"][s] <= ref + gap * sc + 1e-6 * sc, tag + (out["obj"][s], ref)
            else:
                assert abs(out["obj"][s] - ref) <= tol_obj * sc, tag + (out["obj"][s], ref)
            assert out["lower_bound"][s] <= ref + 1e-6 * sc, tag + (out["lower_bound"][s], ref)
            v = out["v"][s]
            assert np.all((v[self.isb] == 0) | (v[self.isb] == 1)), tag
            assert np.all((self.raw["G"] @ v - self.h[s]) / self.rown <= 1e-6), tag
            assert abs(self.value(v, s) - out["obj"][s]) <= 1e-6 * sc, tag + (self.value(v, s), out["obj"][s])

    def close(self):
        self.model.close()


def fuzz_work(seed, N=5, batch=W2_BATCH, **dims):
    mats, d, atoms, rng = fuzz_mld(seed, **dims)
    x0 = rng.standard_normal((batch, d["nx"]))
    om = rng.standard_normal((batch, N * d["nomega"]))
    return Work("fuzz%d_N%d%s" % (seed, N, "".join("_%s%d" % kv for kv in sorted(dims.items()))), mats, d, atoms, N - 1, N, x0, om)


def cfg_work(name, batch, quadratic=False):
    wl = syn.make_workload(name, batch=batch, quadratic=quadratic)
    ag = wl["agents"][0]
    return Work(name + ("q" if quadratic else ""), ag["mats"], ag["dims"], ag["atoms"], wl["N_p"], wl["N_tilde"], ag["x0"], ag["omega"], quadratic)


@pytest.fixture(scope="module")
def w1():
    w = cfg_work("cfg2", 64)
    yield w
    w.close()


@pytest.fixture(scope="module")
def w2():
    ws = [fuzz_work(s) for s in W2_SEEDS]
    yield ws
    for w in ws:
        w.close()


@pytest.fixture(scope="module")
def w3():
    w = cfg_work("cfg2", 16, quadratic=True)
    yield w
    w.close()


def _solve(w, slot=None, monkeypatch=None, reserved=0, **opts):
    """one problem (MLD_SOL_SLOT = slot while it is created), its shape and its results"""
    if slot is None:
        monkeypatch.delenv("MLD_SOL_SLOT", raising=False)
    else:
        monkeypatch.setenv("MLD_SOL_SLOT", slot)
    try:
        p = w.problem(reserved=reserved, **opts)
    finally:
        monkeypatch.delenv("MLD_SOL_SLOT", raising=False)
    shape = p.debug_shape()
    out = w.solve(p)
    p.close()
    return shape, out


_DEFAULT = {}


def _default(w, monkeypatch, reserved=0, **opts):
    """the all-LDS run of the same inputs and options (cached per module)"""
    key = (id(w), reserved, tuple(sorted(opts.items())))
    if key not in _DEFAULT:
        shape, out = _solve(w, None, monkeypatch, reserved, **opts)
        assert shape["all_lds"] and shape["slot_mask"] == 0, (w.name, shape)
        w.check(out, "all-LDS")
        _DEFAULT[key] = (shape, out)
    return _DEFAULT[key]


def _assert_placement(w, slot, shape, base):
    """every array named is in the slot; the shape is otherwise the default's (same dims, same budget)"""
    named = set(SLOT_FIELDS) if slot == "all" else set(slot.split(","))
    for k in ("n", "m0", "mcap", "first_cap", "ld", "mir_cap", "ws_stride", "lds_budget"):
        assert shape[k] == base[k], (w.name, slot, k)
    for nm in named:
        for f in SLOT_FIELDS[nm]:
            assert shape[f] == -1, (w.name, slot, f, shape[f])
    for nm in set(SLOT_FIELDS) - named:       # with less in LDS before it, every other array still fits
        for f in SLOT_FIELDS[nm]:
            assert (shape[f] >= 0) == (base[f] >= 0), (w.name, slot, f, shape[f], base[f])
    moved = any(base[f] >= 0 for nm in named for f in SLOT_FIELDS[nm])
    assert shape["lds_bytes"] < base["lds_bytes"] if moved else shape["lds_bytes"] == base["lds_bytes"], (w.name, slot)


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("obj", "v", "status", "nodes", "pivots"))


def test_unknown_slot_name_is_refused(w2, monkeypatch):
    monkeypatch.setenv("MLD_SOL_SLOT", "xb,lo")
    with pytest.raises(MldGpuError, match="MLD_SOL_SLOT"):
        w2[0].problem()
    monkeypatch.setenv("MLD_SOL_SLOT", "xb,,dw")       # empty items are ignored, names are not
    p = w2[0].problem()
    sh = p.debug_shape()
    p.close()
    assert sh["lXB"] == -1 and sh["lDw"] == -1 and not sh["all_lds"] and sh["slot_mask"] == (1 << 0) | (1 << 7)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# A. placement

HOT_CASES = ("xb", "basic", "skip", "atup", "nonbasic", "xn", "lohi", "dw", "cost")


@pytest.mark.parametrize("slot", HOT_CASES)
def test_hot_array_in_the_slot_is_bit_identical_to_all_lds(slot, w1, w2, monkeypatch):
    """one hot array in the slot: s_dual_simplex_impl<false> (generic pointers), and for `cost` the reduced-cost row behind the dictionary
    (D + mcap * ld).  Only the addresses change, so every result bit is the all-LDS run's."""
    w1_opts = dict(cut_rounds=1) if HOT_CASES.index(slot) % 2 else {}      # half of the cases with one cut round: the search really branches
    for w, opts in [(w1, w1_opts)] + [(w, EXACT) for w in w2]:
        base_shape, base = _default(w, monkeypatch, **opts)
        shape, out = _solve(w, slot, monkeypatch, **opts)
        _assert_placement(w, slot, shape, base_shape)
        assert not shape["all_lds"], (w.name, slot)
        w.check(out, slot)
        assert _same_bits(out, base), (w.name, slot, np.flatnonzero(out["obj"] != base["obj"]), np.flatnonzero(out["pivots"] != base["pivots"]))


MIR_CASES = ("mirline", "mirline,mircache", "lohi,dw,cost,mircache", "lohi,dw,cost,mircache,mirline")


@pytest.mark.parametrize("slot", MIR_CASES)
def test_mir_line_placements_prove_the_highs_optimum(slot, w1, w2, monkeypatch):
    """the c-MIR scoring lines full width in LDS (`mirline`: phase A reads the cache), in the slot (`mirline,mircache`: phase A from the slot and
    phase B block-wide), and cfg5's placement at a small shape.  Each proves the HiGHS optimum; with the serial builder (bit 15) in both runs
    phase B is the same code, so the same number of cuts is made.  (Full-width lines in LDS are bit-identical to the default; with the lines in
    the slot the block-wide phase B rounds differently from a wave per cut, so cfg2's results differ in their last bits there.)"""
    for k, (w, opts) in enumerate([(w1, dict(cut_rounds=1)), (w1, {})] + [(w, EXACT) for w in w2]):
        base_shape, _ = _default(w, monkeypatch, **opts)
        if w is w1:
            assert base_shape["lMirLine"] >= 0 and base_shape["lMirCache"] >= 0      # the default is the compact-line path
        shape, out = _solve(w, slot, monkeypatch, **opts)
        _assert_placement(w, slot, shape, base_shape)
        assert shape["all_lds"] == ("cost" not in slot), (w.name, slot)
        w.check(out, slot)
        print("%s %s: bit-identical to all-LDS: %s" % (slot, w.name, _same_bits(out, _default(w, monkeypatch, **opts)[1])))
        if k == 0 or w is not w1:
            _, sbase = _default(w, monkeypatch, reserved=MIR_SERIAL, **opts)
            _, sout = _solve(w, slot, monkeypatch, reserved=MIR_SERIAL, **opts)
            w.check(sout, slot + " serial")
            assert sout["stats"]["cuts"] == sbase["stats"]["cuts"], (w.name, slot, sout["stats"]["cuts"], sbase["stats"]["cuts"])
            assert sout["stats"]["cuts"] > 0 or w is not w1


def test_everything_in_the_slot(w1, w2, w3, monkeypatch):
    for w, opts in [(w1, dict(cut_rounds=1)), (w3, dict(gap_rel=1e-6, max_nodes=20000, max_pivots=400000))] + [(w, EXACT) for w in w2]:
        base_shape, base = _default(w, monkeypatch, **opts)
        shape, out = _solve(w, "all", monkeypatch, **opts)
        _assert_placement(w, "all", shape, base_shape)
        assert not shape["all_lds"] and all(shape[f] == -1 for f in HOT + ("lMirLine", "lMirCache"))
        w.check(out, "all")
        assert np.array_equal(out["status"], base["status"])


def test_cfg3_sits_at_the_edge_of_the_budget_all_in_lds():
    """cfg3 (7 tanks) at its natural placement: every hot array and both c-MIR line sets in LDS, within 1 KB of the budget -- a budget or
    layout change that pushes it over shows up here"""
    wl = syn.make_workload("cfg3", batch=16)
    ag = wl["agents"][0]
    m = gpu.GpuModel([ag["mats"]], ag["dims"])
    p = gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], ag["dims"], wl["N_p"], wl["N_tilde"]))
    sh = p.debug_shape()
    p.close(); m.close()
    print("cfg3 shape:", sh)
    assert sh["all_lds"] and sh["lMirLine"] >= 0 and sh["lMirCache"] >= 0, sh
    assert 0 <= sh["lds_budget"] - sh["lds_bytes"] <= 1024, sh


# ---------------------------------------------------------------------------------------------------------------------------------------------
# B. diagnostic switches (one handle per model, set_opts(reserved=...))

@pytest.fixture(scope="module")
def handles(w1, w2):
    """one problem per model at gap 0 and its default run; W1 with one cut round (branching), W2 exact"""
    hs = [(w1, w1.problem(cut_rounds=1))] + [(w, w.problem(**EXACT)) for w in w2]
    base = []
    for w, p in hs:
        out = w.solve(p)
        w.check(out, "default")
        base.append(out)
    yield hs, base
    for _, p in hs:
        p.close()


def _run_bit(hs, bit, **opts):
    outs = []
    for w, p in hs:
        keep = {k: getattr(p.opts, k) for k in opts}
        p.set_opts(reserved=bit, **opts)
        try:
            outs.append(w.solve(p))
        finally:
            p.set_opts(reserved=0, **keep)
    return outs


def _total(outs, k):
    return sum(o["stats"][k] for o in outs)


@pytest.mark.parametrize("bit", (1, 2, 3, 5))
def test_speed_only_switches_keep_the_optimum(bit, handles):
    """bits 1-5 change speed and rounding only: same status, objective within 1e-8, and the HiGHS optimum"""
    hs, base = handles
    outs = _run_bit(hs, 1 << bit)
    for (w, _), out, b in zip(hs, outs, base):
        w.check(out, "bit %d" % bit)
        assert np.array_equal(out["status"], b["status"]), (w.name, bit)
        fin = np.isfinite(b["obj"])
        assert np.all(np.abs(out["obj"][fin] - b["obj"][fin]) <= 1e-8 * np.maximum(1.0, np.abs(b["obj"][fin]))), (w.name, bit)
        if bit == 3:                    # queue order: which workgroup solves an instance does not change its bits
            assert _same_bits(out, b), (w.name, bit)
    if bit == 1:
        assert _total(outs, "refactors") > _total(base, "refactors")
    if bit == 2:
        # (these workloads never fail the residual check, so the default refactors no more than bit 2 does: bit 2 is shown to win over bit 1,
        # which refactors at every check)
        assert _total(outs, "refactors") == 0
        both = _run_bit(hs, (1 << 1) | (1 << 2))
        for (w, _), out in zip(hs, both):
            w.check(out, "bits 1 + 2")
        assert _total(both, "refactors") == 0 and _total(_run_bit(hs, 1 << 1), "refactors") > 0
    if bit == 5:
        assert _total(outs, "cuts") > 0


@pytest.mark.parametrize("bit", (6, 13, 14, 15))
def test_search_switches_prove_the_highs_optimum(bit, handles):
    hs, base = handles
    outs = _run_bit(hs, 1 << bit)
    for (w, _), out in zip(hs, outs):
        w.check(out, "bit %d" % bit)
    if bit == 6:
        assert outs[0]["stats"]["nodes"] > hs[0][0].batch, outs[0]["stats"]
    if bit == 15:
        assert _total(outs, "cuts") > 0


def test_serial_mir_with_the_lines_in_the_slot(w1, w2, monkeypatch):
    """bit 15 where the block-wide phase B is the default anyway (the lines in the slot)"""
    for w, opts in [(w1, dict(cut_rounds=1))] + [(w, EXACT) for w in w2]:
        shape, out = _solve(w, "mircache", monkeypatch, reserved=MIR_SERIAL, **opts)
        assert shape["lMirCache"] == -1
        w.check(out, "bit 15 mircache")
        assert out["stats"]["cuts"] > 0 or w is not w1


RESTART_NODES = 100


def test_root_restart_runs_and_the_gap_holds(w1):
    """bit 16 (no root restart) at MIPGap 1e-2 with a node limit low enough (s_root_restart: at least max_nodes / 8 nodes) that searches reach the
    final phase with a gap of 1-3 %: the restart adds cut rounds (the batch's cut count differs with the switch), and either way every instance
    is proven within the gap of HiGHS"""
    p = w1.problem(cut_rounds=1, gap_rel=1e-2, max_nodes=RESTART_NODES)
    on = w1.solve(p)
    p.set_opts(reserved=NO_RESTART)
    off = w1.solve(p)
    p.close()
    print("restart: cuts with %d without %d" % (on["stats"]["cuts"], off["stats"]["cuts"]))
    assert on["stats"]["cuts"] != off["stats"]["cuts"]
    w1.check(on, "restart", gap=1e-2)
    w1.check(off, "bit 16", gap=1e-2)


def test_lazy_mip_start(handles):
    """bit 17: the MIP start evaluated lazily, with the optimal binaries and with an all-zero start"""
    hs, base = handles
    for (w, p), b in zip(hs, base):
        assert np.array_equal(p.is_bin, w.isb)
        opt = np.where(np.isfinite(b["obj"])[:, None], np.rint(b["v"][:, w.isb]), 255).astype(np.uint8)
        p.set_opts(reserved=LAZY_START)
        try:
            for name, start in (("optimal", opt), ("zero", np.zeros_like(opt))):
                w.check(w.solve(p, warm_start=start), "bit 17 %s start" % name)
        finally:
            p.set_opts(reserved=0)


def test_no_closing_sweep_with_the_in_kernel_handoff(w1):
    """bit 19: a stopped search publishes its open nodes without the closing sweep -- with a tiny first pass (as in test_gpu_handoff) the merged
    answer is still the unlimited search's"""
    p = w1.problem(gap_rel=0.0, max_nodes=100000, cut_rounds=1, reserved=NO_SWEEP)
    ref = w1.solve(p)
    w1.check(ref, "bit 19 plain")
    out = p.solve_handoff_device(w1.x0, w1.om, first_nodes=3, sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
    p.close()
    print("bit 19 in-kernel handoff:", out["handoff"])
    assert out["handoff"]["items"] >= 3
    assert np.all(out["status"] == 0), np.unique(out["status"], return_counts=True)
    assert np.allclose(out["obj"], ref["obj"], rtol=1e-9, atol=1e-9)
    assert np.all(out["lower_bound"] <= out["obj"] + 1e-9) and np.all(out["lower_bound"] >= ref["obj"] - 1e-6 * np.maximum(1.0, np.abs(ref["obj"])))
    w1.check(out, "bit 19 hand-off")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# C. cut-row capacity and dictionary shape edges (W2 models of chosen dimensions)

@pytest.mark.parametrize("N, ld_padded", ((9, False), (5, True)))
def test_unpadded_and_padded_rows(N, ld_padded):
    """seed 4 has nv = 7: N = 9 gives n = 63, rows of exactly n + 1 = 64 doubles; N = 5 gives n = 35 in rows of 40"""
    w = fuzz_work(4, N=N, batch=8)
    p = w.problem(**EXACT)
    sh = p.debug_shape()
    assert sh["n"] == 7 * N and (sh["ld"] > sh["n"] + 1) == ld_padded and sh["ld"] % 8 == 0, sh
    w.check(w.solve(p), "ld %d" % sh["ld"])
    p.close(); w.close()


def test_fewer_rows_than_waves():
    w = fuzz_work(0, N=2, batch=8, nc=3)
    p = w.problem(**EXACT)
    sh = p.debug_shape()
    assert sh["m0"] == 6 < 8, sh
    w.check(w.solve(p), "m0 6")
    p.close(); w.close()


def test_more_cut_rows_than_threads():
    w = fuzz_work(1, N=5, batch=8)
    p = w.problem(max_cuts=500, **EXACT)
    sh = p.debug_shape()
    assert sh["mcap"] == sh["m0"] + 500 > 512 and sh["all_lds"], sh
    w.check(w.solve(p), "mcap %d" % sh["mcap"])
    p.close(); w.close()


@pytest.mark.parametrize("max_cuts", (1, 2, 7, 0))
def test_cut_rows_that_fill_in_the_first_round(max_cuts):
    """max_cuts 1, 2, 7: the cut rows are full during the first round; 0 with cut rounds asked for: no cut rows at all (the host drops the rounds)"""
    w = fuzz_work(2, N=5, batch=8)
    p = w.problem(max_cuts=max_cuts, cut_rounds=4, **EXACT)
    sh = p.debug_shape()
    assert sh["mcap"] == sh["m0"] + max_cuts and sh["first_cap"] == sh["mcap"], sh
    out = w.solve(p)
    p.close(); w.close()
    w.check(out, "max_cuts %d" % max_cuts)
    if max_cuts == 0:
        assert out["stats"]["cuts"] == 0 and p.opts.cut_rounds == 0, out["stats"]


@pytest.mark.parametrize("opts", (dict(cuts_per_round=1), dict(mir_per_round=0), dict(mir_per_round=1)))
def test_one_cut_per_round_and_few_rounding_cuts(opts, w2):
    for w in w2[:3]:
        p = w.problem(**EXACT)
        p.set_opts(**opts)
        out = w.solve(p)
        p.close()
        w.check(out, str(opts))
