"""The rows' update of one pivot of k_solve and of a fused pair, alone: the internal entry mld_debug_update_rows builds the sector and row lists
as the solver does and runs the update on a caller-supplied dictionary, with the templates the default loop runs (s_update_rows_r7 / s_update_rows2_r7)
and with the earlier ones (mld_opts.reserved bit 28, MLD_DBG_UPDATE_R7).  The kernel holds both in one instantiation and chooses at run time, as s_pivot
does: the default loop's own inlined copy is what tests/test_gpu_update_paths.py runs.

Both paths must agree BIT FOR BIT with each other and with a host reference whose fused multiply-add is exact (fractions.Fraction, rounded once):
every entry of a row with a non-zero multiplier, on the pivot row's active 64-byte sectors, becomes fma(-mu, rowr[k], old) with the entering
column's old entry counted as 0 -- for a pair the first pivot's update, then the second's, each where its own row and sector flags say so.  Every
other entry of the dictionary must keep its bits.  The (row, sector) pairs the kernel accounts must equal the reference's count.

Shapes: 73 sectors (ld = 584, the benchmark's), of which 1, 15, 16, 17, 33, 48, 49, 64 or 65 are active -- one to five groups of 16 sectors, full
and partial last groups, one chunk of four groups and a second one -- and 1, RB - 1, RB, RB + 1, 8 RB or 8 RB + 1 rows with a non-zero multiplier,
RB being the rows a wave takes at a time for that number of groups (mld_debug_update_shape reports the templates' own constants: 16, 16, 10, 8 today).  8 RB + 1 multipliers need more than 64
rows: the dictionary has 8 * 16 + 5 = 133 (the two pivot rows and two rows with a multiplier of -0.0 besides).  The entering column sits in the even and in the odd slot of its lane, in the first, the last and a
middle active sector, so that it falls into every group.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from pyhybridcontrol_amd import gpu
from pyhybridcontrol_amd._lib import MLD_DBG_UPDATE_R7

pytestmark = pytest.mark.gpu

NSEC, SEC = 73, 8
LD = NSEC * SEC
M = 8 * 16 + 5
ACTIVE = (1, 15, 16, 17, 33, 48, 49, 64, 65)


def _fma(a, b, c):
    """a * b + c rounded once (IEEE-754 binary64, round to nearest even), signed zeros as the hardware gives them"""
    if a == 0.0 or b == 0.0:
        if c != 0.0:
            return c
        neg_p = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        return -0.0 if (neg_p and math.copysign(1.0, c) < 0) else 0.0
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # (an exact sum of 0 from non-zero terms is +0)


def _active(rowr, n):
    return np.array([np.any(rowr[s * SEC:min((s + 1) * SEC, n + 1)] != 0.0) for s in range(NSEC)])


def _apply(D, rows, secs, colc, rowr, c):
    """one pivot's update of `rows` x `secs`, in place"""
    for i in rows:
        mu = float(colc[i])
        for s in secs:
            for k in range(s * SEC, (s + 1) * SEC):
                D[i, k] = _fma(-mu, float(rowr[k]) if k < rowr.size else 0.0, 0.0 if k == c else float(D[i, k]))


def _reference(D, n, p1, p2=None):
    """(updated copy, (row, sector) pairs) -- p = (rowr, colc, r, c)"""
    out = D.copy()
    rowr1, colc1, r1, c1 = p1
    a1 = np.flatnonzero(_active(rowr1, n))
    if p2 is None:
        rows1 = [i for i in range(M) if i != r1 and colc1[i] != 0.0]
        _apply(out, rows1, a1, colc1, rowr1, c1)
        return out, len(rows1) * len(a1)
    rowr2, colc2, r2, c2 = p2
    a2 = np.flatnonzero(_active(rowr2, n))
    rows1 = [i for i in range(M) if i != r1 and i != r2 and colc1[i] != 0.0]
    rows2 = [i for i in range(M) if i != r2 and colc2[i] != 0.0]
    _apply(out, rows1, a1, colc1, rowr1, c1)
    _apply(out, rows2, a2, colc2, rowr2, c2)
    both_r, both_s = len(set(rows1) & set(rows2)), len(set(a1.tolist()) & set(a2.tolist()))
    return out, len(rows1) * len(a1) + len(rows2) * len(a2) - both_r * both_s


def _values(rng, size):
    """full-mantissa doubles of mixed sign and magnitude"""
    return rng.standard_normal(size) * np.exp2(rng.integers(-6, 7, size))


def _dictionary(rng):
    D = _values(rng, (M, LD))
    z = rng.random((M, LD))
    D[z < 0.02] = 0.0
    D[z > 0.98] = -0.0
    return D


def _row(rng, secs, n, c):
    """a staged pivot row whose active sectors are exactly `secs`: some zeros inside them, rowr[c] != 0"""
    rowr = np.zeros(n + 1)
    for s in secs:
        ks = np.arange(s * SEC, min((s + 1) * SEC, n + 1))
        v = _values(rng, ks.size)
        v[rng.random(ks.size) < 0.3] = 0.0
        if not np.any(v != 0.0):
            v[rng.integers(ks.size)] = 1.5
        rowr[ks] = v
    if c is not None:
        rowr[c] = 1.0 / 3.0 + rng.random()
    return rowr


def _column(rng, rows):
    colc = np.zeros(M)
    colc[rows] = _values(rng, len(rows))
    return colc


def _check(D, n, p1, p2, tag):
    ref, ref_pairs = _reference(D, n, p1, p2)
    new, cnt_new = gpu.debug_update_rows(D, n, *p1, second=p2, reserved=0)
    old, cnt_old = gpu.debug_update_rows(D, n, *p1, second=p2, reserved=MLD_DBG_UPDATE_R7)
    u = lambda a: a.view(np.uint64)
    touched = int((u(ref) != u(D)).sum())
    print("%s: %d (row, sector) pairs, %d entries changed; default vs bit 28 differ in %d entries, default vs reference in %d" % (
        tag, ref_pairs, touched, int((u(new) != u(old)).sum()), int((u(new) != u(ref)).sum())))
    assert np.array_equal(u(new), u(old)), (tag, "paths differ at", np.argwhere(u(new) != u(old))[:4].tolist())
    assert np.array_equal(u(new), u(ref)), (tag, "default differs from the exact reference at", np.argwhere(u(new) != u(ref))[:4].tolist())
    assert np.array_equal(u(old), u(ref)), (tag, "bit 28 differs from the exact reference at", np.argwhere(u(old) != u(ref))[:4].tolist())
    assert cnt_new == cnt_old == ref_pairs, (tag, cnt_new, cnt_old, ref_pairs)
    assert touched > 0, tag


@pytest.fixture(scope="module")
def shape():
    s = gpu.debug_update_shape()
    # (the row-block sizes come from the templates' own constexpr through the query: the edges below move with them)
    assert len(s["RB"]) == 4 and all(2 <= rb and s["waves"] * rb + 5 <= M for rb in s["RB"]), s
    assert s["sectors_per_group"] * SEC * 8 == 1024 and s["sector_doubles"] == SEC and s["groups_per_chunk"] == 4, s
    return s


def _row_counts(shape, nact):
    ngrp = -(-nact // shape["sectors_per_group"])
    rbs = sorted({shape["RB"][min(g, 4) - 1] for g in ({ngrp} if ngrp <= 4 else {4, ngrp - 4})})      # (five groups: a chunk of four, then one of one)
    return sorted({k for rb in rbs for k in (1, rb - 1, rb, rb + 1, 8 * rb, 8 * rb + 1)})


@pytest.mark.parametrize("nact", ACTIVE)
def test_one_pivot(shape, nact):
    rng = np.random.default_rng(1000 + nact)
    n = LD - 1
    case = 0
    for nrows in _row_counts(shape, nact):
        for odd in (0, 1):
            secs = np.sort(rng.choice(NSEC, nact, replace=False))
            pos = (0, nact - 1, nact // 2)[case % 3]
            c = int(secs[pos]) * SEC + 2 * int(rng.integers(SEC // 2)) + odd
            if c >= n:
                c -= 2
            r = int(rng.integers(M))
            rows = rng.choice([i for i in range(M) if i != r], nrows, replace=False)
            D, rowr, colc = _dictionary(rng), _row(rng, secs, n, c), _column(rng, rows)
            colc[r] = 2.5      # (the pivot element: the pivot row itself is never in the list)
            _check(D, n, (rowr, colc, r, c), None, "one pivot, %d sectors, %d rows, column %d (%s slot, sector %d of the list)" % (nact, nrows, c, "odd" if odd else "even", pos))
            case += 1


def test_one_pivot_with_padding_columns(shape):
    """n + 1 is no multiple of 8: the last sector ends in padding, which the staged row holds as 0"""
    rng = np.random.default_rng(7)
    n = LD - 5
    secs = np.sort(np.r_[rng.choice(NSEC - 1, 20, replace=False), NSEC - 1])
    c, r = int(secs[3]) * SEC + 1, 5
    rows = rng.choice([i for i in range(M) if i != r], 40, replace=False)
    _check(_dictionary(rng), n, (_row(rng, secs, n, c), _column(rng, rows), r, c), None, "one pivot, padding")


@pytest.mark.parametrize("columns", ("apart", "one_sector", "same_column"))
@pytest.mark.parametrize("nact", ACTIVE)
def test_pair(shape, nact, columns):
    """the union of both pivot rows has `nact` active sectors, flagged 1 (first row only), 2 or 3; rows take the first update, the second or both"""
    rng = np.random.default_rng(2000 + 10 * nact + len(columns))
    n = LD - 1
    rb = _row_counts(shape, nact)
    for k, nrows in enumerate((rb[3], rb[-1])):      # RB + 1 of the smaller block, 8 RB + 1 of the larger
        secs = np.sort(rng.choice(NSEC, nact, replace=False))
        flag = rng.integers(1, 4, nact)
        flag[rng.integers(nact)] = 3
        if nact >= 3:
            flag[:3] = rng.permutation(3) + 1
        s1, s2 = secs[(flag & 1) != 0], secs[(flag & 2) != 0]
        if s1.size == 0 or s2.size == 0:      # (one sector: both rows have it)
            s1 = s2 = secs
        c1 = int(s1[rng.integers(s1.size)]) * SEC + int(rng.integers(SEC))
        if columns == "apart":
            c2 = int(s2[rng.integers(s2.size)]) * SEC + int(rng.integers(SEC))
        else:
            if c1 // SEC not in s2.tolist():
                s2 = np.sort(np.r_[s2, c1 // SEC])
            c2 = c1 if columns == "same_column" else (c1 // SEC) * SEC + (c1 % SEC + 3) % SEC
        c1, c2 = min(c1, n - 1), min(c2, n - 1)
        r1, r2 = (int(x) for x in rng.choice(M, 2, replace=False))
        others = [i for i in range(M) if i not in (r1, r2)]
        rows = rng.choice(others, nrows, replace=False)
        rf = rng.integers(1, 4, nrows)
        rf[:3] = (1, 2, 3)[:min(3, nrows)]
        colc1, colc2 = _column(rng, rows[(rf & 1) != 0]), _column(rng, rows[(rf & 2) != 0])
        colc1[r1], colc2[r2], colc1[r2] = 2.5, -1.75, 0.375      # (the pivot elements; row r2 is never in the list)
        if k == 0:
            colc2[r1] = 0.8125      # r1 inside the list: it takes the second update only
        minus0 = [i for i in others if i not in rows.tolist()][:2]
        colc1[minus0[0]] = -0.0      # a multiplier of -0.0 is no multiplier
        colc2[minus0[1]] = -0.0
        rowr1, rowr2 = _row(rng, s1, n, c1), _row(rng, s2, n, c2)
        _check(_dictionary(rng), n, (rowr1, colc1, r1, c1), (rowr2, colc2, r2, c2),
               "pair (%s), %d sectors (%d / %d), %d rows, columns %d and %d" % (columns, nact, s1.size, s2.size, nrows, c1, c2))


@pytest.mark.parametrize("nact", (33, 48, 49, 64, 65))
def test_pair_entering_columns_in_chosen_groups(shape, nact):
    """three groups or more: the second pivot's entering column is put, on purpose, into every group of the list in turn (the first pivot's into the first and
    into the last group), so that it is found in slot 0, in slot 1 and in a later slot that has to trade places with slot 1"""
    rng = np.random.default_rng(3000 + nact)
    n = LD - 1
    spg = shape["sectors_per_group"]
    ngrp = -(-nact // spg)
    nrows = _row_counts(shape, nact)[3]
    for g1 in (0, ngrp - 1):
        for g2 in range(ngrp):
            secs = np.sort(rng.choice(NSEC, nact, replace=False))      # every sector in both rows: position in the list = position in either row
            p1 = min(g1 * spg + int(rng.integers(spg)), nact - 1)
            p2 = min(g2 * spg + int(rng.integers(spg)), nact - 1)
            c1 = min(int(secs[p1]) * SEC + int(rng.integers(SEC)), n - 1)
            c2 = min(int(secs[p2]) * SEC + int(rng.integers(SEC)), n - 1)
            r1, r2 = (int(x) for x in rng.choice(M, 2, replace=False))
            rows = rng.choice([i for i in range(M) if i not in (r1, r2)], nrows, replace=False)
            rf = rng.integers(1, 4, nrows)
            colc1, colc2 = _column(rng, rows[(rf & 1) != 0]), _column(rng, rows[(rf & 2) != 0])
            colc1[r1], colc2[r2] = 2.5, -1.75
            _check(_dictionary(rng), n, (_row(rng, secs, n, c1), colc1, r1, c1), (_row(rng, secs, n, c2), colc2, r2, c2),
                   "pair, %d sectors, column 1 in group %d, column 2 in group %d" % (nact, g1, g2))
