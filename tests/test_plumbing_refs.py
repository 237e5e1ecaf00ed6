"""The CPU references of tests/test_gpu_batch_plumbing.py checked on their own (no GPU): the plant-update reference against the x(1) block
row of the condensed maps, the MIP-start reference against its two closed forms, and the merge reference against trees merged by hand."""
import numpy as np
import pytest

import _plumbing as pl
import condense_np as cn
from _paths import fuzz_mld

N = 5


@pytest.mark.parametrize("seed", range(12))
def test_advance_ref_is_the_x1_block_row_of_the_condensed_maps(seed):
    mats, dims, _, rng = fuzz_mld(seed)
    nx, nw = dims["nx"], dims["nomega"]
    nv = dims["nu"] + dims["ndelta"] + dims["nz"] + dims["nmu"]
    evo = cn.condense(mats, N)
    B = 4
    x0, om, v = rng.standard_normal((B, nx)), rng.standard_normal((B, N * nw)), rng.standard_normal((B, N * nv))
    status, obj = np.array([0, 2, 1, 2]), np.array([1.0, -2.0, np.inf, np.inf])
    x1, om1, bound, aux, ok = pl.advance_ref([mats], dims, N, x0, om, v, status, obj)
    assert ok.tolist() == [True, True, False, False]
    for b in range(B):
        if not ok[b]:
            assert np.array_equal(x1[b], x0[b]) and np.array_equal(om1[b], om[b])
            continue
        r1 = slice(nx, 2 * nx)      # x(1): the condensed maps' block row 0 is x(0) = x0 itself (Phi_x[:nx] = I, Gamma[:nx] = 0)
        assert np.array_equal(evo["Phi_x"][:nx], np.eye(nx)) and not evo["Gamma_v"][:nx].any()
        ref = evo["Phi_x"][r1] @ x0[b] + evo["Gamma_v"][r1, :nv] @ v[b][:nv] + evo["Gamma_5"][r1, 0]
        if nw:
            ref = ref + evo["Gamma_omega"][r1, :nw] @ om[b][:nw]
        assert np.all(np.abs(x1[b] - ref) <= 2.0 * bound[b] + 1e-300), (seed, b)
        assert np.all(bound[b] > 0) and np.all(bound[b] <= 1e-13 * (1.0 + np.abs(ref).max() + np.abs(x0[b]).max() + np.abs(v[b]).max() * 10))
        assert np.array_equal(om1[b].reshape(N, nw), np.roll(om[b].reshape(N, nw), -1, axis=0))
        nu, nd, nz = dims["nu"], dims["ndelta"], dims["nz"]
        want = np.abs(mats["B2"] @ v[b][nu:nu + nd] + mats["B3"] @ v[b][nu + nd:nu + nd + nz]).max() if nd + nz else 0.0
        assert abs(aux[b] - want) <= 1e-12
    assert pl.fp64_dot_bound(10) == pytest.approx(10 * 2.0 ** -53, rel=1e-12)


def test_warm_ref_closed_forms():
    rng = np.random.default_rng(3)
    nv, B = 5, 6
    step_bin = np.array([0, 1, 1, 0, 1], bool)
    is_bin = np.tile(step_bin, N)
    v = rng.random((B, N * nv))
    v[:, is_bin] = np.rint(v[:, is_bin])
    v[0, is_bin] += 1e-9 * rng.standard_normal(int(is_bin.sum()))          # (a vertex is 0 / 1 up to the LP's tolerance)
    status, obj = np.array([0, 0, 2, 2, 1, 3]), np.array([1.0, -1.0, 5.0, np.inf, np.inf, 2.0])
    w0 = pl.warm_ref(v, status, obj, is_bin, nv, N, 0)
    ok = pl.usable_plan(status, obj)
    assert ok.tolist() == [True, True, True, False, False, False]
    assert np.array_equal(w0[ok], np.rint(v[:, is_bin])[ok].astype(np.uint8)) and np.all(w0[~ok] == 255)
    last = np.rint(v.reshape(B, N, nv)[:, -1, :][:, step_bin]).astype(np.uint8)
    for shift in (N - 1, N, N + 3):
        w = pl.warm_ref(v, status, obj, is_bin, nv, N, shift)
        assert np.array_equal(w[ok].reshape(-1, N, 3), np.repeat(last[ok][:, None, :], N, axis=1))
    w1 = pl.warm_ref(v, status, obj, is_bin, nv, N, 1)
    assert np.array_equal(w1[ok].reshape(-1, N, 3)[:, :-1], w0[ok].reshape(-1, N, 3)[:, 1:])
    assert np.array_equal(w1[ok].reshape(-1, N, 3)[:, -1], last[ok])
    assert pl.warm_rows_equal(w1, w1) and not pl.warm_rows_equal(w1, w0)
    junk = w1.copy(); junk[3, 1:] = 7
    assert pl.warm_rows_equal(junk, w1)
    junk[3, 0] = 0
    assert not pl.warm_rows_equal(junk, w1)


def test_merge_ref_reproduces_trees_merged_by_hand():
    q = pl.hand_queue()
    m = pl.merge_ref(q, gap_abs=0.5, gap_rel=0.0)
    # root 0: items A, B tie at 7 (B has the smaller label), C found nothing: proven, bound max(4, 7 - 0.5)
    # root 1: ties with its item D at -3 (keeps its own point); D stopped at its limit with bound -6: NODE_LIMIT, bound max(-8, min(-6, -3.5))
    # root 2: its own rest is open, nothing found anywhere: NODE_LIMIT without a point, its own bound stands
    # root 3: given up for a full queue: keeps 5 / 2 / its point and counters although item G found 1
    # root 4: was not split
    assert m["status"].tolist() == [0, 2, 2, 2, 0]
    assert m["obj"].tolist() == [7.0, -3.0, np.inf, 5.0, 2.0]
    assert m["lower_bound"].tolist() == [6.5, -6.0, 1.0, 2.0, 2.0]
    assert m["v"][:, 0].tolist() == [6.0, 1.0, 2.0, 3.0, 4.0]
    assert m["nodes"].tolist() == [11, 31, 8, 1, 1] and m["pivots"].tolist() == [22, 62, 16, 2, 2]
    assert m["rows"].tolist() == [11 << 33, 31 << 33, 8 << 33, 1 << 33, 1 << 33]
    assert m["n_unfinished"] == 3 and m["given_up"] == (0, 1)
    # a relative gap: root 0's bound becomes max(4, 7 - 0.25 * 7)
    assert pl.merge_ref(q, gap_abs=1e-9, gap_rel=0.25)["lower_bound"][0] == 5.25
    # the same tree with A unfinished (bound 4.5): not proven, bound max(4, min(4.5, 6.5))
    q2 = pl.hand_queue(); q2["status"][5] = 3; q2["lbnd"][5] = 4.5
    m2 = pl.merge_ref(q2, gap_abs=0.5)
    assert m2["status"][0] == 2 and m2["lower_bound"][0] == 4.5 and m2["obj"][0] == 7.0 and m2["v"][0, 0] == 6.0 and m2["n_unfinished"] == 4
    # ... and with A's bound above the incumbent's gap: the incumbent closes everything above 7 - 0.5, so the bound is min(6.8, 6.5)
    q2["lbnd"][5] = 6.8
    assert pl.merge_ref(q2, gap_abs=0.5)["lower_bound"][0] == 6.5
    # nothing finite in a closed tree: INFEASIBLE
    q3 = pl.hand_queue(); q3["obj"][[0, 5, 6]] = np.inf; q3["status"][[5, 6]] = 1
    m3 = pl.merge_ref(q3, gap_abs=0.5)
    assert m3["status"][0] == 1 and m3["obj"][0] == np.inf and m3["lower_bound"][0] == 4.0 and m3["v"][0, 0] == 0.0
    # -0.0 is below +0.0: the item's point wins over a root at +0.0
    q4 = pl.hand_queue(); q4["obj"][0] = 0.0; q4["obj"][5] = -0.0; q4["obj"][6] = 0.0; q4["lbnd"][[0, 5, 6]] = -1.0
    m4 = pl.merge_ref(q4, gap_abs=0.5)
    assert np.signbit(m4["obj"][0]) and m4["v"][0, 0] == 5.0


def test_merge_ref_on_signed_zeros_denormals_and_last_bit_neighbours():
    m = pl.merge_ref(pl.edge_queue())
    up, dn = np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)
    want = [-0.0, -0.0, -5e-324, dn, -up, np.inf]
    assert np.array_equal(m["obj"].view(np.uint64), np.array(want).view(np.uint64))
    assert m["v"][:, 0].tolist() == [6.5, 1.0, 10.5, 12.5, 15.5, 5.0]       # items 6, 10, 12, 15 win; root 1 ties with item 9 and keeps its point
    assert m["status"].tolist() == [0, 0, 0, 0, 0, 1] and m["n_unfinished"] == 0
    assert m["lower_bound"][:5].tolist() == [-1e-9, -1e-9, -1e-9, dn - 1e-9, -up - 1e-9] and m["lower_bound"][5] == -2.0


@pytest.mark.parametrize("seed", range(6))
def test_merge_ref_does_not_depend_on_the_item_order_and_keeps_its_invariants(seed):
    q = pl.random_queue(seed, batch=40, n_items=600, n=3, cap=700)
    a = pl.merge_ref(q, gap_abs=1e-3, gap_rel=1e-2)
    ok, what = pl.merge_equal(a, pl.merge_ref(pl.shuffle_items(q, seed + 100), gap_abs=1e-3, gap_rel=1e-2))
    assert ok, what
    ok, what = pl.merge_equal(a, pl.merge_ref(pl.hand_queue()))
    assert not ok
    f = pl.queue_facts(q)
    assert f["items"] == 600 and f["tie2"] >= 3 and f["root_tie"] >= 1 and f["dead"] >= 1 and f["neg"] >= 3 and f["big_label"] >= 50
    merged = np.isin(q["status"][:40], (16, 18)) & (q["tree_dead"] == 0)
    assert np.all(a["lower_bound"][merged] <= a["obj"][merged])
    assert np.all(np.isinf(a["obj"][merged & (a["status"] == 1)]))
    assert not np.any(np.isin(a["status"], (16, 17, 18)))
    # the hand queue shuffled as well
    ok, what = pl.merge_equal(pl.merge_ref(pl.hand_queue(), 0.5), pl.merge_ref(pl.shuffle_items(pl.hand_queue(), 1), 0.5))
    assert ok, what
