"""CPU references for the device kernels between solves (tests/test_gpu_batch_plumbing.py): the plant update and forecast shift of
mld_advance_batch2, the MIP start of mld_warm_start_from_previous, and the in-kernel hand-off's merge written per root from its contract
(include/mldgpu.h) -- plain numpy / Python loops in fp64.  Checked on their own by tests/test_plumbing_refs.py."""
import numpy as np

U64 = 2.0 ** -53            # unit roundoff of fp64 (round to nearest)
OPTIMAL, INFEASIBLE, NODE_LIMIT, NUMERICAL, UNBOUNDED = 0, 1, 2, 3, 4
EXPANDED, SKIPPED, EXPANDED_OPEN = 16, 17, 18       # internal statuses of the in-kernel hand-off (never leave the library)
NO_POINT = 1.0e300          # an objective at or above it means "no incumbent"


def usable_plan(status, obj):
    """an instance has a plan to apply when its solve ended OPTIMAL, or at a limit with an incumbent"""
    status, obj = np.asarray(status), np.asarray(obj, np.float64)
    return ((status == OPTIMAL) | (status == NODE_LIMIT)) & (np.abs(obj) < NO_POINT)


def fp64_dot_bound(K):
    """relative bound (times sum_j |a_j z_j|) of a length-K fp64 dot product in any summation order, with or without FMA:
    gamma_K = K u / (1 - K u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)"""
    return K * U64 / (1.0 - K * U64)


def step_rows(mats, dims):
    """[A B1 B2 B3 B4 b5]: the rows of x+ over z = [x; u; delta; z; w_0; 1]"""
    nx = dims["nx"]
    blocks = [np.asarray(mats[k], np.float64).reshape(nx, -1) for k in ("A", "B1", "B2", "B3", "B4")]
    return np.hstack(blocks + [np.asarray(mats["b5"], np.float64).reshape(nx, 1)])


def advance_ref(mats_list, dims, N, x0, omega, v, status, obj, model_idx=None):
    """x+ = A x + B1 u + B2 d + B3 z + B4 w_0 + b5 with (u, d, z) the step-0 slice of v, forecast rolled by one step; instances without a usable
    plan keep both.  Returns (x1, omega1, bound, aux, usable): bound = per element 2 gamma_K sum_j |a_ij z_j| (K = nx + nv + nw + 1: the kernel also
    multiplies the zero columns under mu; the factor 2 is this reference's own rounding), aux = per instance max_i |B2 d0 + B3 z0|_i."""
    nx, nu, nd, nz, nw = dims["nx"], dims["nu"], dims["ndelta"], dims["nz"], dims["nomega"]
    nv = nu + nd + nz + dims["nmu"]
    B = np.shape(v)[0]
    x0 = np.asarray(x0, np.float64).reshape(B, nx)
    omega = np.asarray(omega, np.float64).reshape(B, N * nw)
    ok = usable_plan(status, obj)
    x1, om1, bound, aux = x0.copy(), omega.copy(), np.zeros((B, nx)), np.zeros(B)
    g = 2.0 * fp64_dot_bound(nx + nv + nw + 1)
    for b in range(B):
        if not ok[b]:
            continue
        mats = mats_list[int(model_idx[b]) if model_idx is not None else 0]
        M = step_rows(mats, dims)
        w0 = omega[b].reshape(N, nw)[0] if nw else np.zeros(0)
        zvec = np.concatenate([x0[b], v[b][:nu + nd + nz], w0, [1.0]])
        x1[b] = M @ zvec
        bound[b] = g * (np.abs(M) @ np.abs(zvec))
        if nx and nd + nz:
            aux[b] = np.abs(M[:, nx + nu:nx + nu + nd + nz] @ v[b][nu:nu + nd + nz]).max()
        if nw:
            om1[b] = np.roll(omega[b].reshape(N, nw), -1, axis=0).reshape(-1)
    return x1, om1, bound, aux, ok


def warm_ref(v, status, obj, is_bin, nv, N, shift):
    """warm[b, k] = v[b, min(step + shift, N - 1) nv + pos] > 0.5 for binary k at (step, pos); first byte 255 without a usable plan (the rest of such
    a row is not specified: compare it through `rows_equal`)"""
    bins = np.flatnonzero(np.asarray(is_bin))
    ok = usable_plan(status, obj)
    B = np.shape(v)[0]
    out = np.zeros((B, bins.size), np.uint8)
    for b in range(B):
        if not ok[b]:
            out[b] = 255
            continue
        for k, j in enumerate(bins):
            step, pos = int(j) // nv, int(j) % nv
            out[b, k] = 1 if v[b][min(step + shift, N - 1) * nv + pos] > 0.5 else 0
    return out


def warm_rows_equal(got, ref):
    """exact equality where there is a start; where there is none only the first byte (255) is promised"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return False
    if ref.shape[1] == 0:
        return True
    none = ref[:, 0] == 255
    return bool(np.array_equal(got[~none], ref[~none]) and np.all(got[none, 0] == 255))


# ---- the hand-off merge ---------------------------------------------------------------------------------------------------------------
def _order(x):
    """total order of the doubles the merge takes its minimum in: by value, -0.0 before +0.0"""
    x = float(x)
    return (x, 0 if np.signbit(x) else 1)


def merge_tol(o, gap_abs, gap_rel):
    return max(gap_abs, gap_rel * abs(o)) if o < NO_POINT else 0.0


def merge_ref(q, gap_abs=1e-9, gap_rel=0.0):
    """the merged roots of queue q (dict: batch, tail, obj, lbnd, status, nodes, pivots, cuts, refac, rows, v, item_root, item_label, tree_dead),
    per root, from the contract: see the module docstring of tests/test_gpu_batch_plumbing.py.  Returns the dict gpu.debug_merge returns."""
    B, tail = int(q["batch"]), int(q["tail"])
    obj, lb = np.array(q["obj"][:B], np.float64), np.array(q["lbnd"][:B], np.float64)
    status = np.array(q["status"][:B], np.int32)
    cnt = {k: np.array(q[k][:B], np.int32 if k != "rows" else np.int64) for k in ("nodes", "pivots", "cuts", "refac", "rows")}
    v = np.array(np.asarray(q["v"], np.float64).reshape(len(q["obj"]), -1)[:B])
    vin = np.asarray(q["v"], np.float64).reshape(len(q["obj"]), -1)
    items = {}
    for it in range(B, tail):
        items.setdefault(int(q["item_root"][it]), []).append(it)
    unfinished, gave = 0, [0, 0]
    for r in range(B):
        dead, st = int(q["tree_dead"][r]), int(q["status"][r])
        if dead:
            if st in (EXPANDED, EXPANDED_OPEN):
                status[r] = NODE_LIMIT
            unfinished += 1
            gave[dead - 1] += 1
            continue
        if st not in (EXPANDED, EXPANDED_OPEN):
            continue
        mine = items.get(r, [])
        for k in cnt:
            cnt[k][r] += sum(int(q[k][it]) for it in mine)
        o = min([float(q["obj"][r])] + [float(q["obj"][it]) for it in mine], key=_order)
        fin = o < NO_POINT
        if fin and _order(q["obj"][r]) != _order(o):
            win = min((it for it in mine if _order(q["obj"][it]) == _order(o)), key=lambda it: int(q["item_label"][it]) % 2 ** 64)
            v[r] = vin[win]
        obj[r] = o
        open_lb = [float(q["lbnd"][it]) for it in mine if int(q["status"][it]) in (NODE_LIMIT, NUMERICAL, EXPANDED_OPEN)]
        tol = merge_tol(o, gap_abs, gap_rel)
        lb_r = float(q["lbnd"][r])
        if not open_lb and st == EXPANDED:
            status[r] = OPTIMAL if fin else INFEASIBLE
            if fin:
                lb[r] = min(o, max(lb_r, o - tol))
        else:
            status[r] = NODE_LIMIT
            unfinished += 1
            if st == EXPANDED_OPEN:
                lb[r] = min(lb_r, o if fin else np.inf)
            else:
                lb[r] = max(lb_r, min(min(open_lb, key=_order), o - tol if fin else np.inf))
    return dict(obj=obj, lower_bound=lb, status=status, v=v, n_unfinished=unfinished, given_up=(gave[0], gave[1]), **cnt)


def merge_equal(a, b):
    """bit equality of two merge results (floats compared through their bits: -0.0 is not +0.0)"""
    for k in ("obj", "lower_bound", "v"):
        x, y = np.ascontiguousarray(a[k], np.float64), np.ascontiguousarray(b[k], np.float64)
        if x.shape != y.shape or not np.array_equal(x.view(np.uint64), y.view(np.uint64)):
            return False, k
    for k in ("status", "nodes", "pivots", "cuts", "refac", "rows"):
        if not np.array_equal(a[k], b[k]):
            return False, k
    for k in ("n_unfinished", "given_up"):
        if tuple(np.atleast_1d(a[k])) != tuple(np.atleast_1d(b[k])):
            return False, k
    return True, None


def shuffle_items(q, seed):
    """the same queue with its items in another order (every per-entry array permuted alike over [batch, tail))"""
    B, tail = int(q["batch"]), int(q["tail"])
    perm = np.arange(len(q["obj"]))
    perm[B:tail] = B + np.random.default_rng(seed).permutation(tail - B)
    out = dict(q)
    for k in ("obj", "lbnd", "status", "nodes", "pivots", "cuts", "refac", "rows", "v", "item_root", "item_label"):
        out[k] = np.asarray(q[k])[perm].copy()
    return out


def hand_queue():
    """five roots merged by hand in tests/test_plumbing_refs.py: a proven tree with a tie among its items, a root that ties with an unfinished item, a root whose
    own rest is open and that found nothing, a tree given up for a full queue (dead = 2), a root that was not split; one entry beyond the tail"""
    inf = np.inf
    #        roots: 0      1      2     3     4   | items: A    B    C    D     E    F    G  | beyond the tail
    obj = np.array([10.0, -3.0, inf, 5.0, 2.0,         7.0, 7.0, inf, -3.0, -1.0, inf, 1.0,   -99.0])
    lbnd = np.array([4.0, -8.0, 1.0, 2.0, 2.0,         7.0, 7.0, 5.0, -6.0, -1.0, 3.0, 1.0,   -99.0])
    status = np.array([16, 16, 18, 16, 0,               0,   0,   1,   2,    0,   1,   0,     2], np.int32)
    root = np.array([0, 0, 0, 0, 0,                     0,   0,   0,   1,    1,   2,   3,     0], np.int32)
    label = np.array([0, 0, 0, 0, 0,                    9,   5,   2,   3,    4,   2,   2,     1], np.int64)
    nodes = np.array([5, 1, 1, 1, 1,                    2,   3,   1,   10,   20,  7,   50,    1000], np.int32)
    dead = np.array([0, 0, 0, 2, 0], np.int32)
    v = np.arange(13, dtype=np.float64)[:, None] * np.ones((1, 2))
    return dict(batch=5, tail=12, obj=obj, lbnd=lbnd, status=status, nodes=nodes, pivots=2 * nodes, cuts=0 * nodes, refac=0 * nodes,
                rows=nodes.astype(np.int64) << 33, v=v, item_root=root, item_label=label, tree_dead=dead)


def edge_queue():
    """six split roots with two closed items each, chosen for the order-preserving double -> u64 map: -0.0 against +0.0 (item wins / root ties),
    denormals of both signs, neighbours in the last bit on both sides of +1 and -1, and a tree where nothing is finite.  v row e = e (+ 0.5 for items)."""
    inf, up, dn = np.inf, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)
    #                roots 0..5                      | items of 0    of 1      of 2          of 3    of 4      of 5
    obj = np.array([0.0, -0.0, 5e-324, 1.0, -1.0, inf,   -0.0, 0.0,  0.0, -0.0,  -5e-324, 0.0,  dn, up,  -dn, -up,  inf, inf])
    root = np.array([0, 0, 0, 0, 0, 0,                    0, 0,       1, 1,       2, 2,          3, 3,    4, 4,     5, 5], np.int32)
    label = np.array([0, 0, 0, 0, 0, 0,                   7, 3,       4, 2,       2 ** 40, 5,    9, 8,    3, 2 ** 50, 2, 3], np.int64)
    status = np.array([16] * 6 + [0] * 10 + [1, 1], np.int32)
    one = np.ones(18, np.int32)
    v = (np.arange(18)[:, None] + 0.5 * (np.arange(18)[:, None] >= 6)) * np.ones((1, 3))
    return dict(batch=6, tail=18, obj=obj, lbnd=np.full(18, -2.0), status=status, nodes=one, pivots=one, cuts=one, refac=one, rows=one.astype(np.int64),
                v=v, item_root=root, item_label=label, tree_dead=np.zeros(6, np.int32))


SPECIAL_POOL = np.array([-0.0, 0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), -1.0,
                         np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), -1.5])


def random_queue(seed, batch, n_items, n, cap=None, owners="random", special=0.25, tie_pool=4, dead_share=0.15, root_status=None):
    """a seeded synthetic hand-off queue that is consistent the way a real one is: every root's bound is below every objective of its tree, every
    item's bound is between the root's bound and its own objective, labels are unique, only split roots (given up or not) own items.
    owners: "random" | "one" (every item under root 0: contention on one address) | "each" (item k under split root k mod #split).
    special: share of roots whose objectives come from SPECIAL_POOL (signed zeros, denormals, neighbours in the last bit, negatives);
    tie_pool: distinct finite objectives per ordinary root (small = many ties)."""
    rng = np.random.default_rng(seed)
    cap = int(cap if cap is not None else batch + n_items + 3)
    tail = batch + n_items
    assert cap > batch and tail <= cap
    obj, lbnd = np.full(cap, np.inf), np.full(cap, -np.inf)
    status = np.zeros(cap, np.int32)
    root_status = np.asarray(root_status if root_status is not None else rng.choice([EXPANDED, EXPANDED, EXPANDED_OPEN, OPTIMAL, NODE_LIMIT, INFEASIBLE], batch), np.int32)
    if owners == "one":
        root_status[0] = EXPANDED
    split = np.flatnonzero((root_status == EXPANDED) | (root_status == EXPANDED_OPEN))
    if split.size == 0:
        root_status[0] = EXPANDED
        split = np.array([0])
    dead = np.zeros(batch, np.int32)
    if owners != "one":
        dead[split] = rng.choice([0, 1, 2], split.size, p=[1 - dead_share, dead_share / 2, dead_share / 2])
    pools, base = [], np.zeros(batch)
    for r in range(batch):
        if rng.random() < special:
            pools.append(SPECIAL_POOL)
            base[r] = -2.0
        else:
            base[r] = 20.0 * rng.standard_normal()
            pools.append(base[r] + np.sort(rng.random(tie_pool)) * (1.0 + abs(base[r])))
    status[:batch] = root_status
    for r in range(batch):
        lbnd[r] = base[r]
        inf_ok = root_status[r] != OPTIMAL
        obj[r] = np.inf if (inf_ok and rng.random() < 0.3) else (pools[r].min() if rng.random() < 0.4 else rng.choice(pools[r]))      # (the pool's minimum: root and items tie)
        if root_status[r] == INFEASIBLE:
            obj[r] = np.inf
    item_root = np.zeros(cap, np.int32)
    if n_items:
        item_root[batch:tail] = {"random": lambda: rng.choice(split, n_items), "one": lambda: np.zeros(n_items, np.int32),
                                 "each": lambda: split[np.arange(n_items) % split.size]}[owners]()
    for it in range(batch, tail):
        r = int(item_root[it])
        st = int(rng.choice([OPTIMAL, INFEASIBLE, INFEASIBLE, NODE_LIMIT, NUMERICAL, EXPANDED, SKIPPED, EXPANDED_OPEN], p=[.3, .2, .2, .08, .02, .1, .05, .05]))
        if st in (INFEASIBLE, SKIPPED):
            o = np.inf
        elif st == OPTIMAL or rng.random() < 0.6:
            o = float(rng.choice(pools[r]))
        else:
            o = np.inf
        status[it], obj[it] = st, o
        top = o if np.isfinite(o) else float(pools[r][-1])
        lbnd[it] = base[r] + rng.random() * (top - base[r])
    label = np.zeros(cap, np.int64)
    lab = rng.choice(np.arange(2, 2 + 4 * max(1, n_items)), max(1, n_items), replace=False).astype(np.int64)
    big = rng.random(lab.size) < 0.3
    lab[big] += (np.int64(1) << np.int64(33)) * rng.integers(1, 2 ** 28, int(big.sum()))       # labels above 2^32 (deep positions: 129^gen)
    label[batch:tail] = lab[:n_items]
    ints = lambda hi: rng.integers(0, hi, cap).astype(np.int32)
    nodes, pivots, cuts, refac = ints(1000), ints(100000), ints(50), ints(20)
    rows = rng.integers(0, 2 ** 40, cap).astype(np.int64)
    for a in (nodes, pivots, cuts, refac, rows):
        a[status == SKIPPED] = 0
    v = (np.arange(cap)[:, None] + 0.5 * (np.arange(cap)[:, None] >= batch) + 1e-3 * np.arange(n)[None, :]).astype(np.float64)
    # beyond the tail: values that would win every comparison if they were read
    obj[tail:], lbnd[tail:], status[tail:], item_root[tail:], label[tail:] = -1e9, -1e9, NODE_LIMIT, 0, 1
    return dict(batch=batch, tail=tail, obj=obj, lbnd=lbnd, status=status, nodes=nodes, pivots=pivots, cuts=cuts, refac=refac, rows=rows, v=v,
                item_root=item_root, item_label=label, tree_dead=dead)


def queue_facts(q):
    """what a generated queue contains, for the tests' reach assertions: items, split roots, roots whose best objective is shared by k >= 2 items, roots
    that tie with an item, given-up roots, negative / signed-zero best objectives"""
    B, tail = int(q["batch"]), int(q["tail"])
    f = dict(items=tail - B, split=0, tie2=0, tie5=0, root_tie=0, dead=int((np.asarray(q["tree_dead"]) > 0).sum()), neg=0, zero_pair=0, big_label=0,
             all_inf=0, numerical=0, max_owned=0)
    owned = {}
    for it in range(B, tail):
        owned.setdefault(int(q["item_root"][it]), []).append(it)
    f["big_label"] = int((np.asarray(q["item_label"][B:tail]) > 2 ** 32).sum())
    for r in range(B):
        if int(q["status"][r]) not in (EXPANDED, EXPANDED_OPEN) or q["tree_dead"][r]:
            continue
        f["split"] += 1
        mine = owned.get(r, [])
        f["max_owned"] = max(f["max_owned"], len(mine))
        if not mine:
            continue
        objs = [float(q["obj"][it]) for it in mine]
        o = min(objs + [float(q["obj"][r])], key=_order)
        if not o < NO_POINT:
            f["all_inf"] += 1
            continue
        k = sum(1 for x in objs if _order(x) == _order(o))
        f["tie2"] += k >= 2
        f["tie5"] += k >= 5
        f["root_tie"] += k >= 1 and _order(q["obj"][r]) == _order(o)
        f["neg"] += o < 0
        f["zero_pair"] += (o == 0.0) and any(x == 0.0 and np.signbit(x) != np.signbit(o) for x in objs + [float(q["obj"][r])])
        f["numerical"] += any(int(q["status"][it]) == NUMERICAL for it in mine)
    return f
