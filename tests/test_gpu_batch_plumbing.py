"""The device kernels BETWEEN solves against plain fp64 references (tests/_plumbing.py, checked by tests/test_plumbing_refs.py): k_advance
(mld_advance_batch2), k_warm_from_plan (mld_warm_start_from_previous, read back through the internal entry mld_debug_warm_start),
k_merge_init / a / b / c / d (the in-kernel hand-off's merge, run on synthetic queues through the internal entry mld_debug_merge: the same
function, launch sequence and grid sizes as after k_solve), k_batch_stats and k_pack_results.

The models are tests/_paths.fuzz_mld: dense B2 / B3, so that the planned (delta, z) drive the state -- on the tank clusters every other test
of these kernels uses, those columns of the packed [B1 B2 B3 0] block are multiplied by zeros.

Contract of the merge the reference is written from (include/mldgpu.h), for a root r that was split (internal status 16
EXPANDED or 18 EXPANDED_OPEN) and not given up, over its items: work counters grow by the items' sums; o = min(obj[r], obj[items]) (in the order
of the doubles' bits: -0.0 below +0.0); the point is the root's own if it attains o, else that of the item with the smallest label among those
that attain it; o >= 1e300 = none.  Open items ended NODE_LIMIT, NUMERICAL or EXPANDED_OPEN.  No open item and status 16: OPTIMAL with
lb = min(o, max(lb_r, o - tol)), tol = max(gap_abs, gap_rel |o|), or INFEASIBLE without a finite point; otherwise NODE_LIMIT, counted, with
lb = min(lb_r, o) for status 18 and max(lb_r, min(lb_open, o - tol)) for 16.  A given-up root (tree_dead 1 / 2) keeps everything, turns
NODE_LIMIT if it was 16 / 18, and is counted; a root that was not split is untouched; entries at or beyond the tail are ignored."""
import numpy as np
import pytest

import _plumbing as pl
from _paths import fuzz_mld
from pyhybridcontrol_amd import gpu, host
from pyhybridcontrol_amd._lib import MldGpuError

pytestmark = pytest.mark.gpu

N_P, N = 4, 5
LIMITS = dict(max_nodes=50000, max_pivots=400000)
SAME = dict(nx=2, nu=2, ndelta=1, nz=1, nomega=1, ny=1, nc=4)          # seeds 20..23: four same-shaped models


def _single(seed, nb=6, **fix):
    """one fuzz model, its problem and its nb seeded instances"""
    mats, dims, atoms, rng = fuzz_mld(seed, **fix)
    x0 = rng.standard_normal((nb, dims["nx"]))
    om = rng.standard_normal((nb, N * dims["nomega"]))
    m = gpu.GpuModel([mats], dims)
    p = gpu.GpuProblem(m, N_P, N, host.cost_from_atoms(atoms, dims, N_P, N), **LIMITS)
    return [mats], dims, m, p, x0, om, None


def _four_models(per_model=8, n_problems=1):
    """seeds 20..23 as ONE model set, per_model instances each, model_idx interleaved by a seeded permutation"""
    made = [fuzz_mld(s, **SAME) for s in range(20, 24)]
    dims = made[0][1]
    x0 = np.concatenate([r.standard_normal((per_model, dims["nx"])) for _, _, _, r in made])
    om = np.concatenate([r.standard_normal((per_model, N * dims["nomega"])) for _, _, _, r in made])
    midx = np.repeat(np.arange(4), per_model).astype(np.int32)
    perm = np.random.default_rng(7).permutation(4 * per_model)
    mats_list = [mm for mm, _, _, _ in made]
    m = gpu.GpuModel(mats_list, dims)
    cost = host.stack_costs([host.cost_from_atoms(a, dims, N_P, N) for _, _, a, _ in made])
    ps = [gpu.GpuProblem(m, N_P, N, cost, **LIMITS) for _ in range(n_problems)]
    return mats_list, dims, m, (ps[0] if n_problems == 1 else ps), x0[perm], om[perm], midx[perm]


def _check_advance(mats_list, dims, x0, om, out, p, midx, tag):
    """advance() against the reference; returns (per-instance auxiliary contribution, usable mask, largest |x+ - ref| / bound)"""
    skipped = p.advance()
    x1, om1 = p.inputs()
    rx, rw, bound, aux, ok = pl.advance_ref(mats_list, dims, N, x0, om, out["v"], out["status"], out["obj"], midx)
    assert skipped == int((~ok).sum()), (tag, skipped, int((~ok).sum()))
    err = np.abs(x1 - rx)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0
    print("advance %s: usable %d / %d, max |x+ - ref| / bound = %.3f, max aux %.3g" % (tag, ok.sum(), ok.size, ratio, aux.max() if aux.size else 0.0))
    assert np.all(err <= bound), (tag, ratio)
    assert np.array_equal(x1[~ok], np.asarray(x0).reshape(x1.shape)[~ok]), tag
    assert np.array_equal(om1, rw), tag
    return aux, ok, ratio


# ---- 1. k_advance ---------------------------------------------------------------------------------------------------------------------
def test_advance_on_models_whose_auxiliaries_drive_the_state():
    """all twelve fuzz seeds (nomega = 0: 3, 4, 9, 10; ndelta = 0: 4, 6, 11; nz = 0: 1, 3, 4, 9; ny = 2: 2, 7, 10 -- the offset of [B1 B2 B3 0] in the
    packed model is a sum over the sizes of C, D4, d5, E, F4, f5, G).  Per element |x+ - ref| <= 2 gamma_K sum_j |a_ij z_j|."""
    strong, worst = [], 0.0
    for seed in range(12):
        mats_list, dims, m, p, x0, om, midx = _single(seed)
        out = p.solve(x0, om)
        aux, ok, ratio = _check_advance(mats_list, dims, x0, om, out, p, midx, "seed %d" % seed)
        p.close(); m.close()
        assert ok.all(), (seed, out["status"])          # (tests/test_gpu_fuzz.py: these 72 instances end OPTIMAL)
        worst = max(worst, ratio)
        if aux[ok].max() >= 0.1:
            strong.append(seed)
    print("seeds with max |B2 d0 + B3 z0| >= 0.1:", strong, " largest |x+ - ref| / bound over all seeds: %.3f" % worst)
    assert len(strong) >= 6, strong


def test_advance_several_models_in_one_batch():
    mats_list, dims, m, p, x0, om, midx = _four_models()
    assert len(set(midx[:4].tolist())) > 1          # interleaved
    out = p.solve(x0, om, midx)
    aux, ok, _ = _check_advance(mats_list, dims, x0, om, out, p, midx, "four models")
    p.close(); m.close()
    assert ok.all() and int((aux >= 0.05).sum()) >= 16, (out["status"], aux)
    # the models really differ in what the test looks at: the reference with model 0 for everybody is far off
    wrong = pl.advance_ref(mats_list, dims, N, x0, om, out["v"], out["status"], out["obj"], np.zeros_like(midx))[0]
    right = pl.advance_ref(mats_list, dims, N, x0, om, out["v"], out["status"], out["obj"], midx)[0]
    assert np.abs(wrong - right)[midx != 0].max() > 0.1


def _partly_skipped(p, x0, om, midx):
    """every third instance under a cutoff just below its optimum: INFEASIBLE, infinite objective, no plan"""
    first = p.solve(x0, om, midx)
    assert np.all(first["status"] == 0)
    cut = np.full(len(x0), np.inf)
    cut[::3] = first["obj"][::3] - 1e-6 * np.maximum(1.0, np.abs(first["obj"][::3]))
    p.upload(x0, om, midx)
    p.set_cutoffs(cut)
    stats = p.solve_resident()
    out = p.download()
    assert np.all(out["status"][::3] == 1) and not np.any(np.isfinite(out["obj"][::3]))
    return first, out, stats


def test_advance_and_warm_start_of_a_partly_skipped_batch():
    mats_list, dims, m, p, x0, om, midx = _four_models()
    first, out, _ = _partly_skipped(p, x0, om, midx)
    ok = pl.usable_plan(out["status"], out["obj"])
    assert (~ok).sum() >= 1 and ok.sum() >= len(x0) // 2 and (~ok).sum() == len(x0[::3])
    for shift in (0, 1):         # the start of a batch where some instances have no plan: first byte 255 there
        p.warm_start_from_previous(shift)
        got = p.debug_warm_start()
        assert pl.warm_rows_equal(got, pl.warm_ref(out["v"], out["status"], out["obj"], p.is_bin, m.nv, N, shift)), shift
        assert np.all(got[~ok, 0] == 255) and np.all(got[ok] <= 1)
    aux, ok2, _ = _check_advance(mats_list, dims, x0, om, out, p, midx, "partly skipped")
    assert np.array_equal(ok, ok2)
    x1, om1 = p.inputs()
    assert np.array_equal(x1[~ok], x0[~ok]) and np.array_equal(om1[~ok], om[~ok])
    assert not np.array_equal(om1[ok], om[ok]) and np.all(np.abs(x1[ok] - x0[ok]).max(axis=1) > 0)
    p.close(); m.close()


@pytest.mark.parametrize("batch", [1, 51, 52, 85, 86, 257])
def test_advance_batch_sizes_around_the_block_size(batch):
    """a 3-state model with a one-column disturbance over N = 5 steps: batch nx = 255 / 258 at 85 / 86, batch nW = 255 / 260 at 51 / 52"""
    mats_list, dims, m, p, x6, w6, _ = _single(20, nx=3, nu=2, ndelta=1, nz=1, nomega=1, ny=1, nc=4)
    assert dims["nx"] == 3 and N * dims["nomega"] == 5
    idx = np.arange(batch) % 6
    scale = 1.0 + 0.01 * (np.arange(batch) // 6)[:, None]          # (repeats of the six draws, slightly scaled: every row is its own check)
    x0, om = x6[idx] * scale, w6[idx] * scale
    out = p.solve(x0, om)
    aux, ok, _ = _check_advance(mats_list, dims, x0, om, out, p, None, "batch %d" % batch)
    p.close(); m.close()
    assert ok.sum() * 2 >= batch and aux[ok].max() >= 0.05


def test_advance_without_states_shifts_the_forecast_only():
    """nx = 0 (mld_problem_create accepts such a model): no plant to update -- zero-sized A, B4, b5 in front of the packed [B1 B2 B3 0], one thread
    per (instance, state) with no state -- the forecast still moves on"""
    mats, dims, atoms, rng = fuzz_mld(3, nx=0, nomega=1)
    assert dims["nx"] == 0
    om = rng.standard_normal((6, N))
    m = gpu.GpuModel([mats], dims)
    p = gpu.GpuProblem(m, N_P, N, host.cost_from_atoms(atoms, dims, N_P, N), **LIMITS)
    out = p.solve(None, om)
    ok = pl.usable_plan(out["status"], out["obj"])
    assert ok.sum() >= 3, out["status"]
    assert p.advance() == int((~ok).sum())
    x1, om1 = p.inputs()
    assert x1.shape == (6, 0)
    assert np.array_equal(om1[ok], np.roll(om[ok], -1, axis=1)) and np.array_equal(om1[~ok], om[~ok])
    p.close(); m.close()


@pytest.mark.parametrize("which", ["single", "four_models"])
def test_closed_loop_on_device_equals_a_host_driven_twin(which):
    """four steps of advance() / warm_start_from_previous(1) / solve_resident() against a second handle that is given the first one's inputs and the
    numpy-built start: every result of every step bit-equal (the solver is bit-reproducible)"""
    if which == "single":
        mats_list, dims, m, p, x0, om, midx = _single(5)
        _, _, atoms, _ = fuzz_mld(5)
        q = gpu.GpuProblem(m, N_P, N, host.cost_from_atoms(atoms, dims, N_P, N), **LIMITS)
    else:
        mats_list, dims, m, (p, q), x0, om, midx = _four_models(n_problems=2)
    p.upload(x0, om, midx); p.solve_resident(); a = p.download()
    q.upload(x0, om, midx); q.solve_resident(); b = q.download()
    moved = 0
    for step in range(4):
        for k in ("obj", "status", "v", "nodes", "pivots"):
            assert np.array_equal(a[k], b[k]), (which, step, k)
        assert pl.usable_plan(a["status"], a["obj"]).sum() * 2 >= len(x0), (step, a["status"])
        x_prev, _ = p.inputs()
        p.advance()
        p.warm_start_from_previous(1)
        x, w = p.inputs()
        moved += int(not np.array_equal(x, x_prev))
        start = pl.warm_ref(a["v"], a["status"], a["obj"], p.is_bin, m.nv, N, 1)
        assert pl.warm_rows_equal(p.debug_warm_start(), start)
        q.upload(x, w, midx)
        q.set_warm_start(start)
        assert np.array_equal(q.debug_warm_start(), start)
        p.solve_resident(); a = p.download()
        q.solve_resident(); b = q.download()
    for k in ("obj", "status", "v", "nodes", "pivots"):
        assert np.array_equal(a[k], b[k]), (which, "last", k)
    assert moved == 4
    p.close(); q.close(); m.close()


# ---- 2. k_warm_from_plan, read back ------------------------------------------------------------------------------------------------------
def test_warm_start_from_previous_is_the_shifted_rounded_plan():
    """binaries in u and in delta (fuzz seeds 0, 1, 2, 5, 7) and the four-model batch; shifts 0, 1, N - 1, N, N + 3"""
    changed = []
    cases = [("seed %d" % s, lambda s=s: _single(s)) for s in (0, 1, 2, 5, 7)] + [("four models", _four_models)]
    for tag, make in cases:
        mats_list, dims, m, p, x0, om, midx = make()
        assert dims["nu_l"] > 0 and dims["ndelta"] > 0 and p.n_bin == N * (dims["nu_l"] + dims["ndelta"])
        out = p.solve(x0, om, midx)
        assert np.all(out["status"] == 0)
        ref = {}
        for shift in (0, 1, N - 1, N, N + 3):
            p.warm_start_from_previous(shift)
            got = p.debug_warm_start()
            ref[shift] = pl.warm_ref(out["v"], out["status"], out["obj"], p.is_bin, m.nv, N, shift)
            assert got is not None and np.array_equal(got, ref[shift]), (tag, shift)
        assert np.array_equal(ref[N - 1], ref[N + 3])
        with pytest.raises(MldGpuError):
            p.warm_start_from_previous(-1)
        diff = ref[1] != ref[0]
        if tag == "four models":         # (per model of the set)
            changed += [bool(diff[midx == k].any()) for k in range(4)]
        else:
            changed.append(bool(diff.any()))
        p.close(); m.close()
    print("shift 1 differs from shift 0:", changed)
    assert len(changed) == 9 and sum(changed) >= 4, changed


def test_what_clears_and_what_sets_the_start():
    mats_list, dims, m, p, x0, om, midx = _single(2)
    p.upload(x0, om)
    assert p.debug_warm_start() is None
    with pytest.raises(MldGpuError):
        p.warm_start_from_previous(0)                  # no finished solve
    p.solve_resident()
    p.warm_start_from_previous(0)
    assert p.debug_warm_start() is not None
    p.set_warm_start(None)
    assert p.debug_warm_start() is None
    mine = (np.arange(6 * p.n_bin).reshape(6, p.n_bin) % 2).astype(np.uint8)
    mine[4] = 255
    p.set_warm_start(mine)
    assert np.array_equal(p.debug_warm_start(), mine)
    p.upload(x0, om)                                   # an upload clears it
    assert p.debug_warm_start() is None
    p.solve_resident(); p.warm_start_from_previous(1)
    p.stage(np.stack([x0, 2 * x0]), np.stack([om, om]))
    assert p.debug_warm_start() is not None            # (staging alone changes no input)
    p.select(1)                                        # a selection clears it
    assert p.debug_warm_start() is None
    p.solve_resident(); out = p.download(); p.warm_start_from_previous(0)
    assert p.debug_warm_start() is not None
    p.advance()                                        # an advance clears it; the shifted plan sets it again
    assert p.debug_warm_start() is None
    p.warm_start_from_previous(1)
    assert np.array_equal(p.debug_warm_start(), pl.warm_ref(out["v"], out["status"], out["obj"], p.is_bin, m.nv, N, 1))
    p.close(); m.close()


# ---- 3. the hand-off merge on synthetic queues ---------------------------------------------------------------------------------------------
def _merge(q, **gaps):
    return gpu.debug_merge(q["batch"], q["tail"], q["obj"], q["lbnd"], q["status"], q["nodes"], q["pivots"], q["cuts"], q["refac"], q["rows"], q["v"],
                           q["item_root"], q["item_label"], q["tree_dead"], **gaps)


def _merge_invariants(q, got, gap_abs, gap_rel):
    B = q["batch"]
    merged = np.isin(q["status"][:B], (pl.EXPANDED, pl.EXPANDED_OPEN)) & (q["tree_dead"] == 0)
    o, lb, st = got["obj"][merged], got["lower_bound"][merged], got["status"][merged]
    assert np.all(lb <= o)
    tol = np.array([pl.merge_tol(x, gap_abs, gap_rel) for x in o])
    opt = st == pl.OPTIMAL
    assert np.all(lb[opt] >= o[opt] - tol[opt])          # OPTIMAL: obj - lb <= tol, stated in the rounding of the one subtraction the merge does
    assert np.all(np.isposinf(o[st == pl.INFEASIBLE]))
    assert np.all(np.isin(st, (pl.OPTIMAL, pl.INFEASIBLE, pl.NODE_LIMIT)))


def test_merge_of_trees_merged_by_hand_and_of_the_bit_pattern_edges():
    for q, gaps in ((pl.hand_queue(), dict(gap_abs=0.5, gap_rel=0.0)), (pl.hand_queue(), dict(gap_abs=1e-9, gap_rel=0.25)), (pl.edge_queue(), dict(gap_abs=1e-9, gap_rel=0.0))):
        got, ref = _merge(q, **gaps), pl.merge_ref(q, **gaps)
        ok, what = pl.merge_equal(got, ref)
        assert ok, (what, got[what], ref[what])
        _merge_invariants(q, got, **gaps)
    got = _merge(pl.hand_queue(), gap_abs=0.5)
    assert got["status"].tolist() == [0, 2, 2, 2, 0] and got["lower_bound"].tolist() == [6.5, -6.0, 1.0, 2.0, 2.0] and got["v"][:, 0].tolist() == [6.0, 1.0, 2.0, 3.0, 4.0]
    assert got["n_unfinished"] == 3 and got["given_up"] == (0, 1)
    q = pl.hand_queue(); q["status"][5] = pl.NUMERICAL; q["lbnd"][5] = 6.8       # an unfinished item whose bound lies above the incumbent's gap
    got = _merge(q, gap_abs=0.5)
    assert got["status"][0] == 2 and got["lower_bound"][0] == 6.5 and got["obj"][0] == 7.0 and got["v"][0, 0] == 6.0 and got["n_unfinished"] == 4
    got = _merge(pl.edge_queue())
    assert np.signbit(got["obj"][:2]).all() and got["v"][:, 0].tolist() == [6.5, 1.0, 10.5, 12.5, 15.5, 5.0]


#          batch items  n   cap   owners    what it is there for
QUEUES = [(1,    0,     1,  2,    "random"),    # tail == batch: nothing to merge
          (1,    1,     1,  2,    "one"),       # one item, tail == cap
          (1,    255,   255, 300, "one"),
          (1,    256,   257, 256 + 1, "one"),   # tail == cap; the point copy strides by 256 threads
          (1,    257,   1,  400,  "one"),
          (8,    4000,  5,  4100, "one"),       # thousands of items under one root: contention on one address
          (300,  300,   3,  700,  "each"),      # one item per split root
          (300,  3000,  2,  3300, "random"),    # tail == cap
          (300,  3500,  4,  4396, "random"),
          (37,   900,   2,  1000, "random")]
GAPS = [(1e-9, 0.0), (1.0, 0.0), (1e-9, 1e-2), (1.0, 1e-2)]


def test_merge_on_generated_queues_equals_the_per_root_reference_in_any_item_order():
    facts = {}
    for k, (batch, items, n, cap, owners) in enumerate(QUEUES):
        q = pl.random_queue(100 + k, batch, items, n, cap=cap, owners=owners, tie_pool=3 if k % 2 else 6)
        f = pl.queue_facts(q)
        assert f["items"] == items and q["tail"] == batch + items and len(q["obj"]) == cap
        for key, val in f.items():
            facts[key] = max(facts.get(key, 0), val) if key == "max_owned" else facts.get(key, 0) + val
        for gap_abs, gap_rel in (GAPS if k in (5, 8, 9) else GAPS[k % 4:k % 4 + 1]):
            got, ref = _merge(q, gap_abs=gap_abs, gap_rel=gap_rel), pl.merge_ref(q, gap_abs, gap_rel)
            ok, what = pl.merge_equal(got, ref)
            assert ok, (k, gap_abs, gap_rel, what)
            _merge_invariants(q, got, gap_abs, gap_rel)
            again = _merge(pl.shuffle_items(q, 500 + k), gap_abs=gap_abs, gap_rel=gap_rel)       # the header's promise: the queue order does not enter
            ok, what = pl.merge_equal(got, again)
            assert ok, (k, "shuffled", what)
    print("generated merge queues:", facts)
    assert facts["tie2"] >= 20 and facts["tie5"] >= 5 and facts["root_tie"] >= 5 and facts["neg"] >= 20 and facts["big_label"] >= 1000
    assert facts["dead"] >= 10 and facts["all_inf"] >= 3 and facts["numerical"] >= 5 and facts["max_owned"] >= 4000 and facts["split"] >= 300


def test_merge_reports_every_status_branch():
    """one queue, every way a tree can end, with the counts stated: proven, infeasible, unfinished for an open item, unfinished for the root's own
    rest, given up for its size (+1) and for a full queue (+65536), not split"""
    q = pl.random_queue(10, 64, 100, 3, cap=200, dead_share=0.3)
    got, ref = _merge(q, gap_abs=1e-6, gap_rel=1e-3), pl.merge_ref(q, 1e-6, 1e-3)
    ok, what = pl.merge_equal(got, ref)
    assert ok, what
    split = np.isin(q["status"][:64], (16, 18))
    live = split & (q["tree_dead"] == 0)
    assert got["given_up"] == (int((q["tree_dead"] == 1).sum()), int((q["tree_dead"] == 2).sum())) and min(got["given_up"]) >= 1
    assert got["n_unfinished"] == int((q["tree_dead"] > 0).sum()) + int((got["status"][live] == 2).sum())
    for st in (0, 1, 2):
        assert (got["status"][live] == st).any(), st
    assert (got["status"][live & (q["status"][:64] == 18)] == 2).all() and (q["status"][:64] == 18).sum() >= 3
    keep = ~live
    for k_in, k_out in (("obj", "obj"), ("lbnd", "lower_bound"), ("nodes", "nodes"), ("rows", "rows")):
        assert np.array_equal(got[k_out][keep], q[k_in][:64][keep])
    assert np.array_equal(got["v"][keep], q["v"][:64][keep])
    assert np.all(got["nodes"][live] >= q["nodes"][:64][live]) and (got["nodes"][live] > q["nodes"][:64][live]).any()


def test_merge_entry_refuses_what_would_index_out_of_range():
    def bad(**change):
        q = pl.hand_queue()
        for k, val in change.items():
            if isinstance(val, tuple):
                q[k] = q[k].copy(); q[k][val[0]] = val[1]
            else:
                q[k] = val
        with pytest.raises(MldGpuError):
            _merge(q)
    bad(item_root=(7, 5))            # a root index == batch
    bad(item_root=(7, -1))
    bad(tail=4)                      # tail < batch
    bad(tail=14)                     # tail > cap
    bad(batch=13, tree_dead=np.zeros(13, np.int32))      # cap == batch
    bad(batch=0, tree_dead=np.zeros(0, np.int32))
    bad(tree_dead=(1, 3))
    with pytest.raises(MldGpuError):
        _merge(pl.hand_queue(), gap_abs=-1.0)
    q = pl.hand_queue(); q["item_root"] = q["item_root"].copy(); q["item_root"][12] = 99       # beyond the tail: never read
    ok, what = pl.merge_equal(_merge(q, gap_abs=0.5), pl.merge_ref(pl.hand_queue(), 0.5))
    assert ok, what


# ---- 4. k_batch_stats, k_pack_results, staged inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 255, 256, 257, 1000])
def test_batch_stats_are_the_sums_and_counts_of_the_downloaded_results(batch):
    """repeats of the six instances of fuzz seed 2, every third under a cutoff below its optimum (INFEASIBLE).  None of the fuzz seeds 0..11 has an
    unbounded instance at this horizon (HiGHS), so UNBOUNDED is not in the mix; n_numerical is compared all the same."""
    mats_list, dims, m, p, x6, w6, _ = _single(2)
    idx = np.arange(batch) % 6
    first, out, stats = _partly_skipped(p, x6[idx], w6[idx], None)
    p.close(); m.close()
    st = out["status"]
    assert stats["nodes"] == int(out["nodes"].astype(np.int64).sum()) and stats["pivots"] == int(out["pivots"].astype(np.int64).sum())
    assert stats["n_optimal"] == int((st == 0).sum()) and stats["n_infeasible"] == int((st == 1).sum())
    assert stats["n_node_limit"] == int((st == 2).sum()) and stats["n_numerical"] == int((st >= 3).sum())
    assert stats["n_infeasible"] == len(idx[::3]) and stats["n_optimal"] + stats["n_infeasible"] + stats["n_node_limit"] + stats["n_numerical"] == batch
    assert stats["pivots"] > 0 and (batch < 3 or stats["n_optimal"] > 0)


def test_gather_rows_of_a_model_with_continuous_auxiliaries_and_slacks():
    """k_pack_results through a one-rank communicator: 257 instances of fuzz seed 5 (nz = 2, nmu = 4: the step-0 slice is [u delta z mu] of a model
    that is not laid out like a tank), every third without a point (infinite objective)"""
    from pyhybridcontrol_amd import _lib
    from pyhybridcontrol_amd.batch import RcclGather
    mats_list, dims, m, p, x6, w6, _ = _single(5)
    assert dims["nz"] > 0 and dims["nmu"] > 0
    idx = np.arange(257) % 6
    first, out, _ = _partly_skipped(p, x6[idx], w6[idx], None)
    g = RcclGather(1, 0, RcclGather.unique_id())
    try:
        rows = g.gather_results(p)
    finally:
        _lib.load().mld_comm_destroy()
    p.close(); m.close()
    assert rows.shape == (1, 257, 2 + m.nv)
    assert np.array_equal(rows[0, :, 0], out["obj"]) and np.isinf(rows[0, ::3, 0]).all() and np.isfinite(rows[0, 1::3, 0]).all()
    assert np.array_equal(rows[0, :, 1], out["status"].astype(float))
    assert np.array_equal(rows[0, :, 2:], out["v"][:, :m.nv])
    assert np.abs(rows[0, 1::3, 2 + dims["nu"] + dims["ndelta"]:2 + dims["nu"] + dims["ndelta"] + dims["nz"]]).max() > 0        # the z columns carry values


def test_staged_inputs_without_a_disturbance_and_after_an_advance():
    """nomega = 0 (fuzz seed 3): zero-width forecast through stage / select / inputs / advance"""
    mats_list, dims, m, p, x0, om, _ = _single(3)
    assert dims["nomega"] == 0 and p.nW == 0
    sets = np.stack([x0, -x0, 0.5 * x0 + 1.0])
    p.upload(x0, om)
    assert p.stage(sets, np.zeros((3, 6, 0))) == 3
    for k in (2, 0, 1):
        p.select(k)
        x, w = p.inputs()
        assert np.array_equal(x, sets[k]) and w.shape == (6, 0)
        with pytest.raises(MldGpuError):
            p.advance()                                 # a selection has not been solved
        p.solve_resident(); got = p.download()
        ref = p.solve(sets[k], om)
        assert np.array_equal(got["obj"], ref["obj"]) and np.array_equal(got["v"], ref["v"])
        p.select(k); p.solve_resident(); out = p.download()
        _check_advance(mats_list, dims, sets[k], om, out, p, None, "staged set %d" % k)
        with pytest.raises(MldGpuError):
            p.advance()                                 # the plan has been applied
    p.select(1)                                         # the staged sets are untouched by the advances
    assert np.array_equal(p.inputs()[0], sets[1])
    p.close(); m.close()
