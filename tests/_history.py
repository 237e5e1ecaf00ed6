"""Helpers of the history tests (tests/test_gpu_history.py; checked by tests/test_history_host.py): does a solve's answer depend on what its workgroup
solved before?  k_solve is a persistent workgroup that solves one queue entry after another in the same Shared struct, the same LDS and the same
workspace slot; DESIGN section 4 promises that "a solve is bit-reproducible whatever slot, batch position or launch it runs in".  Here:

* all_pairs_sequence(k): a sequence over range(k) in which every ordered pair of kinds (a, a) included is a pair of neighbours -- with one slot and the
  queue in upload order, "kind a directly before kind b in the same workgroup" is then covered for all a, b;
* P35: six hard-row models of EQUAL dimensions (one multi-model handle), six instances each, classified by HiGHS with the margin guard of tests/_hard.py;
* p35_inputs: per-instance inputs for the pool (MIP starts, fixings, cutoffs, a per-instance linear cost) with what HiGHS says of each altered instance;
* chain(kinds): the upload order that applies the sequence to a pool whose instances carry kinds;
* assert_same_bits: every chain position against the single solve of its instance, through uint64 views; assert_anchor: against HiGHS.

CPU only: numpy and scipy."""
import numpy as np

import _hard
import condense_np as cn
from _paths import fuzz_mld

KEYS = ("obj", "v", "lower_bound", "status", "nodes", "pivots", "rows_updated")      # per instance; "cuts" and "refactors" are compared as totals

P35_DIMS = dict(nx=3, nu=2, ndelta=2, nz=2, nomega=1, ny=2, nc=6)
P35_SEEDS = range(6)
P35_N, P35_NP, P35_NB = 5, 4, 6


# ---- the sequence -------------------------------------------------------------------------------------------------------------------------------
def all_pairs_sequence(k):
    """an Eulerian circuit of the complete digraph on k vertices with loops (every vertex has k arcs in and k out, so one exists), as its vertex
    sequence: length k * k + 1, every ordered pair (a, b) of range(k) occurs as (seq[i], seq[i + 1]) exactly once.  Hierholzer's algorithm."""
    k = int(k)
    if k < 1:
        raise ValueError("all_pairs_sequence: k >= 1")
    nxt = [0] * k                 # the next unused arc of vertex a goes to nxt[a]
    stack, out = [0], []
    while stack:
        a = stack[-1]
        if nxt[a] < k:
            stack.append(nxt[a])
            nxt[a] += 1
        else:
            out.append(stack.pop())
    return out[::-1]


def pairs_of(labels):
    """the set of ordered neighbour pairs of a sequence of labels"""
    return set(zip(labels[:-1], labels[1:]))


def chain(kinds_of_instances, reverse=False):
    """the upload order that runs all_pairs_sequence over the kinds present: returns (order, kinds) with order an int array of instance numbers of
    length k * k + 1 and kinds the sorted list of distinct labels.  The instances of a kind are taken round-robin and may repeat."""
    kinds = sorted(set(kinds_of_instances), key=repr)
    members = {lab: [i for i, x in enumerate(kinds_of_instances) if x == lab] for lab in kinds}
    taken = dict.fromkeys(kinds, 0)
    order = []
    for a in all_pairs_sequence(len(kinds)):
        lab = kinds[a]
        order.append(members[lab][taken[lab] % len(members[lab])])
        taken[lab] += 1
    order = np.asarray(order[::-1] if reverse else order, np.int64)
    return order, kinds


def covered(order, kinds_of_instances):
    """(pairs of kinds that are neighbours in the order, number of kinds present)"""
    labs = [kinds_of_instances[i] for i in order]
    return pairs_of(labs), len(set(labs))


def assert_all_pairs(order, kinds_of_instances, required=()):
    """every required kind is present in the chain and every ordered pair of the kinds present is a pair of neighbours; returns the number of pairs"""
    pairs, _ = covered(order, kinds_of_instances)
    present = sorted(set(kinds_of_instances[i] for i in order), key=repr)
    for r in required:
        assert r in present, ("the chain lacks kind", r, present)
    missing = [(a, b) for a in present for b in present if (a, b) not in pairs]
    assert not missing, ("ordered pairs of kinds that are never neighbours", missing[:6])
    return len(pairs)


# ---- the pool -------------------------------------------------------------------------------------------------------------------------------------
_cache = {}


def p35(N=P35_N):
    """P35: fuzz_mld(seed, nx=3, nu=2, ndelta=2, nz=2, nomega=1, ny=2, nc=6) for seeds 0-5, rows 1.. hard, N_tilde = 5, N_p = 4 (n = 35, 30 rows, 20
    binaries), six instances per model drawn as _hard.family_instances draws them.  Returns dict(models = [dict(mats, dims, atoms, raw, rs)], dims, N_p,
    N, x0 (36, nx), om (36, N nomega), midx (36,), inst = [the classification of _hard.classify with h, q, r, model]).  Computed once.
    Another N gives the same models and x0 at that horizon (N_p = N - 1), unclassified (cls None): the LP tests use N = 12."""
    if ("p35", N) in _cache:
        return _cache[("p35", N)]
    models, x0s, oms, midx, inst = [], [], [], [], []
    for k, seed in enumerate(P35_SEEDS):
        mats, dims, atoms, rng = fuzz_mld(seed, **P35_DIMS)
        mats, dims, atoms = _hard.hard_variant(mats, dims, atoms, range(1, dims["nc"]))
        x0 = 1.5 * rng.standard_normal((P35_NB, dims["nx"]))
        om = rng.standard_normal((P35_NB, N * dims["nomega"]))
        raw = cn.standard_form(mats, atoms, N - 1, N, nu_l=dims["nu_l"])
        models.append(dict(mats=mats, dims=dims, atoms=atoms, raw=raw, rs=_hard.row_scale(raw["G"])))
        for s in range(P35_NB):
            h, q = cn.rhs(raw["evo"], x0[s], om[s]), cn.lin_cost(raw["cost"], x0[s], om[s])
            c = _hard.classify(raw, h, q) if N == P35_N else dict(cls=None)
            c.update(h=h, q=q, r=cn.cost_const(raw["cost"]["const_terms"], x0[s], om[s]), model=k)
            inst.append(c)
        x0s.append(x0); oms.append(om); midx += [k] * P35_NB
    pool = dict(models=models, dims=models[0]["dims"], N_p=N - 1, N=N, x0=np.concatenate(x0s), om=np.concatenate(oms),
                midx=np.asarray(midx, np.int32), inst=inst)
    _cache[("p35", N)] = pool
    return pool


def classes(inst):
    """(feasible, infeasible, dropped) of a list of classifications"""
    cl = [c["cls"] for c in inst]
    return cl.count("feasible"), cl.count("infeasible"), cl.count("dropped")


def _with(raw, bins, fixed):
    """the standard form with the binaries fixed where `fixed` is not 255"""
    lb, ub = raw["lb"].copy(), raw["ub"].copy()
    on = fixed != 255
    lb[bins[on]] = ub[bins[on]] = fixed[on].astype(float)
    return dict(raw, lb=lb, ub=ub)


FEASIBLE_VARIANTS = ("own_start", "bad_start", "no_start", "fix_partial", "fix_contra", "cut_above", "cut_below")
INFEASIBLE_VARIANTS = ("no_start", "bad_start", "fix_partial")


def p35_inputs():
    """per-instance inputs of P35 for the chain that mixes them.  Every instance gets a row of each array (a batch has one layout), the neutral value where
    its variant does not use it: warm (36, 20) uint8 (255 first = no start), fixed (36, 20) uint8 (255 = free), cutoff (36,) (inf = none), lin_v (36, 35)
    (zero on a seeded half of the instances, and on the binaries only: the cost of the free auxiliaries is left alone, so boundedness is that of the pool).
    variant[i] names what instance i got, the feasible instances in turn

        own_start    the start is HiGHS's optimal binaries            bad_start   a start HiGHS's LP cannot complete within the margin (violated[i];
                                                                                  "other_start" where neither all-zero nor all-one is one)
        no_start     nothing                                          fix_partial every third binary fixed at its optimal value
        fix_contra   one binary fixed so that HiGHS finds the MILP infeasible beyond the margin
        cut_above    cutoff = optimum + 1e-3 s                        cut_below   cutoff = optimum - 1e-3 s   (s = max(1, |optimum|), the constant included)

    and the infeasible ones no_start / bad_start (all zero) / fix_partial (every third binary at 0).  expect[i] is the classification of the ALTERED
    instance (cost q + lin_v, bounds with the fixings): cls "feasible" with opt / lo / r, "infeasible", "dropped", or "cut_below" (status INFEASIBLE:
    nothing better than the cutoff).  kind[i] = variant, "+lin" with a non-zero cost row, "/inf" on an instance of the pool that is infeasible."""
    if "inputs" in _cache:
        return _cache["inputs"]
    pool = p35()
    nI = len(pool["inst"])
    raw0 = pool["models"][0]["raw"]
    bins = np.where(raw0["is_bin"])[0]
    nb, n = len(bins), raw0["G"].shape[1]
    rng = np.random.default_rng(3535)
    has_lin = rng.permutation(nI) < nI // 2
    warm, fixed = np.full((nI, nb), 255, np.uint8), np.full((nI, nb), 255, np.uint8)
    cutoff, lin_v = np.full(nI, np.inf), np.zeros((nI, n))
    variant, expect, violated = [None] * nI, [None] * nI, np.zeros(nI, bool)
    turn = {"feasible": 0, "infeasible": 0}
    for i, c in enumerate(pool["inst"]):
        raw = pool["models"][c["model"]]["raw"]
        assert np.array_equal(np.where(raw["is_bin"])[0], bins)
        if has_lin[i]:
            lin_v[i, bins] = 0.5 * rng.standard_normal(nb)
        q = c["q"] + lin_v[i]
        e = _hard.classify(raw, c["h"], q) if has_lin[i] else {k: c[k] for k in ("cls", "opt", "lo", "x") if k in c}
        e["r"] = c["r"]
        if e["cls"] == "dropped":
            variant[i], expect[i] = "no_start", e
            continue
        names = FEASIBLE_VARIANTS if e["cls"] == "feasible" else INFEASIBLE_VARIANTS
        name = names[turn[e["cls"]] % len(names)]
        turn[e["cls"]] += 1
        if e["cls"] == "infeasible":
            if name == "bad_start":
                warm[i] = 0
            elif name == "fix_partial":
                fixed[i, ::3] = 0
            variant[i], expect[i] = name, e
            continue
        xb = np.rint(e["x"][bins]).astype(np.uint8)
        s = max(1.0, abs(e["opt"] + e["r"]))
        if name == "own_start":
            warm[i] = xb
        elif name == "bad_start":
            for val in (0, 1):
                warm[i] = val
                k = _hard.classify_lp(raw, c["h"], q, *[_with(raw, bins, warm[i])[b] for b in ("lb", "ub")])
                if k["cls"] == "infeasible":
                    violated[i] = True
                    break
            else:
                name = "other_start"          # (HiGHS can complete both the all-zero and the all-one start: a start, but none that violates a hard row)
        elif name == "fix_partial":
            fixed[i, ::3] = xb[::3]
        elif name == "fix_contra":
            loose = c["h"] + _hard.MARGIN * _hard.row_scale(raw["G"])      # (infeasible with every row loosened by the margin: _hard.classify's "infeasible")
            for k in range(nb):
                f = np.full(nb, 255, np.uint8)
                f[k] = 1 - xb[k]
                if _hard._milp(_with(raw, bins, f), loose, q).status == 2:
                    fixed[i] = f
                    e = dict(cls="infeasible", r=c["r"])
                    break
            else:
                name = "no_start"          # (no single binary contradicts this instance beyond the margin)
        elif name == "cut_above":
            cutoff[i] = e["opt"] + e["r"] + 1e-3 * s
        elif name == "cut_below":
            cutoff[i] = e["opt"] + e["r"] - 1e-3 * s
            e = dict(cls="cut_below", r=c["r"])
        variant[i], expect[i] = name, e
    kind = [variant[i] + ("+lin" if has_lin[i] else "") + ("/inf" if pool["inst"][i]["cls"] == "infeasible" else "") for i in range(nI)]
    out = dict(warm=warm, fixed=fixed, cutoff=cutoff, lin_v=lin_v, variant=variant, expect=expect, violated=violated, kind=kind)
    _cache["inputs"] = out
    return out


def p35_lp_fixings(seed=35, N=P35_N):
    """every binary of every instance of p35(N) fixed at a seeded random value, and the class of each LP by scipy's linprog with the margin guard
    (_hard.classify_lp): (fixed (36, 4 N) uint8, [classification with r])"""
    if ("lp", seed, N) in _cache:
        return _cache[("lp", seed, N)]
    pool = p35(N)
    bins = np.where(pool["models"][0]["raw"]["is_bin"])[0]
    fixed = (np.random.default_rng([seed, 35 if N == P35_N else N]).random((len(pool["inst"]), len(bins))) < 0.5).astype(np.uint8)
    inst = []
    for i, c in enumerate(pool["inst"]):
        raw = pool["models"][c["model"]]["raw"]
        b = _with(raw, bins, fixed[i])
        k = _hard.classify_lp(raw, c["h"], c["q"], b["lb"], b["ub"])
        k["r"] = c["r"]
        inst.append(k)
    _cache[("lp", seed, N)] = (fixed, inst)
    return fixed, inst


# ---- the comparisons ------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same_bits(chain_out, alone_out, order, tag, kinds=None, keys=KEYS):
    """chain_out: the results of a batch uploaded in `order` (arrays with one row per position, rows_updated among them, and "stats", the launch's
    mld_stats); alone_out: the same arrays with one row per INSTANCE of the pool, each row from that instance's single solve, plus per-instance
    "cuts" and "refactors".  Every key of `keys` is compared bit for bit (float64 through uint64 views: -0.0 and NaN payloads count), position by
    position; the failure names position, instance, its kind and the kind uploaded before it.  Then the cuts / refactors totals."""
    order = np.asarray(order)
    bad = []
    for k in keys:
        a, b = _bits(chain_out[k]), _bits(np.asarray(alone_out[k])[order])
        assert a.shape == b.shape, (tag, k, a.shape, b.shape)
        for pos in np.flatnonzero(np.any((a != b).reshape(len(order), -1), axis=1)):
            bad.append((int(pos), k))
    if bad:
        bad.sort()
        pos, k = bad[0]
        i = int(order[pos])
        kind = (lambda j: kinds[j]) if kinds is not None else (lambda j: "?")
        first = "%s: position %d (instance %d, kind %r, after %s) differs from its single solve in %r: chain %r, alone %r" % (
            tag, pos, i, kind(i), "nothing" if pos == 0 else "instance %d of kind %r" % (int(order[pos - 1]), kind(int(order[pos - 1]))), k,
            _short(chain_out[k][pos]), _short(np.asarray(alone_out[k])[i]))
        raise AssertionError("%s; %d (position, key) pairs differ in all: %s" % (first, len(bad), bad[:12]))
    for k in ("cuts", "refactors"):
        if k in alone_out:
            want = int(np.asarray(alone_out[k])[order].sum())
            assert int(chain_out["stats"][k]) == want, (tag, k, "chain total", int(chain_out["stats"][k]), "sum of the single solves", want)


def _short(x):
    x = np.asarray(x)
    return x.tolist() if x.size <= 4 else "array of %d, first %s" % (x.size, x.ravel()[:4].tolist())


def assert_anchor(out, order, expect, tag):
    """every position against HiGHS's verdict on its instance: INFEASIBLE exactly on the instances classified infeasible (and under a cutoff below
    the optimum), status 0 inside _hard.sandwich on the feasible ones; nothing on the dropped ones.  Returns (feasible, infeasible) positions checked."""
    n_f = n_i = 0
    for pos, i in enumerate(np.asarray(order)):
        e, st, obj = expect[int(i)], int(out["status"][pos]), float(out["obj"][pos])
        what = (tag, pos, int(i), e["cls"], st, obj)
        if e["cls"] == "dropped":
            continue
        if e["cls"] in ("infeasible", "cut_below"):
            assert st == 1, what
            n_i += 1
            continue
        assert st == 0, what
        ok, rel = _hard.sandwich(e, obj)
        assert ok, what + (e["lo"] + e["r"], e["opt"] + e["r"], rel)
        n_f += 1
    return n_f, n_i
