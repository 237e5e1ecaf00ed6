"""A toy device for GpuProblem.solve_handoff (no GPU): small binary trees with enumerated leaves, searched depth first with the kernel's stack
protocol under the uploaded fixings, cutoff and node limit, as include/mldgpu.h describes a solve (mld_set_cutoffs, mld_download_open_nodes).
solve_handoff reaches the device only through record_open_nodes, set_opts, solve, open_nodes, upload, set_cutoffs, solve_resident and download;
ToyProblem is a GpuProblem made without __init__ that answers those from the trees (solve stays the inherited upload + solve_resident +
download), so the bookkeeping under test is the real one and the optimum of every tree is known by enumeration.

stack_dfs is the one depth-first search with that stack protocol: test_host's partition test of expand_open_nodes drives it with random
branching, the toy with bounds and an incumbent."""
import types

import numpy as np

from pyhybridcontrol_amd import MldGpuError, gpu

FREE = 255


def stack_dfs(fix0, enter, choose, leaf):
    """Depth-first search over the free (255) entries of fix0 with the solver's stack: one entry [variable, current value, sibling accounted for]
    per level.  enter(a) is asked at every node (a = the node's fixings): "stop" ends the search THERE -- the current path is still open -- and
    the stack is returned; "prune" closes the node; anything else goes on.  choose(a, rest) -> (variable, first value, closed_other) branches a
    node with free entries `rest` (closed_other: the sibling is closed without a node of its own, as penalty branching does now and then);
    leaf(a) sees every full assignment that is reached.  Returns None when the search ran to its end."""
    fix0 = np.asarray(fix0, dtype=np.uint8)
    stack = []

    def rec():
        a = fix0.copy()
        for v_, val_, _ in stack:
            a[v_] = val_
        verdict = enter(a)
        if verdict == "stop":
            return [list(e) for e in stack]
        if verdict == "prune":
            return None
        rest = [int(j) for j in np.flatnonzero(a == FREE)]
        if not rest:
            leaf(a)
            return None
        j, first, closed_other = choose(a, rest)
        stack.append([int(j), int(first), 1 if closed_other else 0])
        st = rec()
        if st is not None:
            return st
        if not closed_other:
            stack[-1][1], stack[-1][2] = 1 - int(first), 1
            st = rec()
            if st is not None:
                return st
        stack.pop()
        return None

    return rec()


class ToyTree(object):
    """nb binaries, a value per full assignment (some inf), some binaries fixed from the start (the fixed_bin the batch is solved with).
    bound(a) = min over the node's leaves of the relaxed value (the leaf's own, or a finite phantom where the leaf is inf: a relaxation is
    feasible where no integer point is) minus the slack weights of the node's free binaries: never above the node's best leaf, exact at a
    leaf, and it only grows down the tree."""

    def __init__(self, seed, nb, n_free, all_inf=False, dive_first=False):
        rng = np.random.default_rng(seed)
        self.seed, self.nb = int(seed), int(nb)
        self.bits = ((np.arange(2 ** nb)[:, None] >> np.arange(nb)[None, :]) & 1).astype(np.uint8)
        self.leaf = rng.integers(0, 60, size=2 ** nb).astype(np.float64) * 0.5          # a coarse grid: ties happen
        self.leaf[rng.random(2 ** nb) < 0.3] = np.inf
        if all_inf:
            self.leaf[:] = np.inf
        self.relaxed = np.where(np.isfinite(self.leaf), self.leaf, rng.integers(0, 60, size=2 ** nb) * 0.5)
        self.w = rng.uniform(0.0, 1.5, size=nb)
        self.base = np.full(nb, FREE, np.uint8)
        for j in rng.choice(nb, size=nb - n_free, replace=False):
            self.base[j] = rng.integers(0, 2)
        self.dive_first = bool(dive_first) and np.isfinite(self.optimum())
        self._bound = {}

    def mask(self, a):
        a = np.asarray(a, dtype=np.uint8)
        return np.all((self.bits == a[None, :]) | (a[None, :] == FREE), axis=1)

    def min_leaf(self, a):
        return float(self.leaf[self.mask(a)].min())

    def optimum(self):
        return self.min_leaf(self.base)

    def bound(self, a):
        key = np.asarray(a, dtype=np.uint8).tobytes()
        if key not in self._bound:
            free = np.asarray(a) == FREE
            self._bound[key] = self.min_leaf(a) if not free.any() else float(self.relaxed[self.mask(a)].min() - self.w[free].sum())
        return self._bound[key]

    def leaf_of(self, bits):
        return float(self.leaf[int((np.asarray(bits, dtype=np.int64) << np.arange(self.nb)).sum())])

    def branch_rng(self, a):
        return np.random.default_rng([self.seed, int.from_bytes(np.asarray(a, dtype=np.uint8).tobytes(), "little")])


class ToyProblem(gpu.GpuProblem):
    """The device side of solve_handoff on ToyTrees.  An instance is a tree (x0 carries its index) under fixings; the decision vector is one
    continuous entry (the leaf's value) followed by the nb binaries, so the stack's variable index is not the binary position.
    inject = "unsplit" / "status4": in the first hand-off pass a tree with several nodes and a finite optimum is taken (the pick-th of them), of
    its nodes the one with the smallest bound, and every solve of that node comes back unsplit (NODE_LIMIT, depth -1) / UNBOUNDED (4).  log collects what the tests' reach assertions need."""

    @classmethod
    def make(cls, trees, gap_abs=0.0, max_nodes=1000, inject=None, pick=0):
        p = cls.__new__(cls)
        nb = trees[0].nb
        p.trees = list(trees)
        p.model = types.SimpleNamespace(dims=dict(nx=1))
        p.nW, p.n_bin, p.n = 0, nb, nb + 1
        p.is_bin = np.array([False] + [True] * nb)
        p.opts = types.SimpleNamespace(max_nodes=int(max_nodes), gap_rel=0.0, gap_abs=float(gap_abs))
        p._h, p.batch = None, 0
        p.recording, p.inject, p.pick, p.injected = False, inject, int(pick), None
        p.log = dict(passes=0, first_status=None, injected_returns=0, dropped_beside_open=0, cutoffs_cleared=False)
        return p

    # -- what solve_handoff calls ----------------------------------------------------------------
    def record_open_nodes(self, enable=True):
        self.recording = bool(enable)

    def set_opts(self, **opts):
        for k, v in opts.items():
            if not hasattr(self.opts, k):
                raise TypeError("option %r cannot be changed on an existing problem" % k)
            setattr(self.opts, k, type(getattr(self.opts, k))(v))

    def upload(self, x0, omega, model_idx=None, fixed_bin=None):
        x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 1)
        self.batch = x0.shape[0]
        self.inst = np.rint(x0[:, 0]).astype(np.int64)
        self.fix = (np.full((self.batch, self.n_bin), FREE, np.uint8) if fixed_bin is None
                    else np.array(fixed_bin, dtype=np.uint8).reshape(self.batch, self.n_bin))
        self.cut = np.full(self.batch, np.inf)                  # an upload clears the cutoffs
        self.res = None
        return self.batch

    def set_cutoffs(self, cutoff):
        self.log["cutoffs_cleared"] = cutoff is None
        self.cut = np.full(self.batch, np.inf) if cutoff is None else np.array(cutoff, dtype=np.float64).reshape(self.batch)

    def solve_resident(self):
        b, nb = self.batch, self.n_bin
        first_pass = self.log["passes"] == 0
        self.log["passes"] += 1
        if self.inject and self.injected is None and not first_pass:
            cand = [t for t in dict.fromkeys(int(t) for t in self.inst) if (self.inst == t).sum() >= 2 and np.isfinite(self.trees[t].optimum())]
            if cand:
                t = cand[self.pick % len(cand)]
                s = min(np.flatnonzero(self.inst == t), key=lambda s_: (self.trees[t].bound(self.fix[s_]), self.trees[t].min_leaf(self.fix[s_])))
                self.injected = (t, self.fix[s].tobytes())
        res = dict(v=np.zeros((b, self.n)), obj=np.full(b, np.inf), status=np.zeros(b, np.int32), lower_bound=np.zeros(b),
                   nodes=np.zeros(b, np.int32), pivots=np.zeros(b, np.int32), depth=np.full(b, -1, np.int32),
                   var=np.zeros((b, nb), np.int16), val=np.zeros((b, nb), np.uint8), flag=np.zeros((b, nb), np.uint8))
        hit = None
        for s in range(b):
            tree = self.trees[int(self.inst[s])]
            if self.injected == (int(self.inst[s]), self.fix[s].tobytes()):
                hit = s
                self.log["injected_returns"] += 1
                res["nodes"][s], res["pivots"][s] = 1, 7
                if self.inject == "status4":
                    res["obj"][s], res["status"][s], res["lower_bound"][s] = -np.inf, 4, -np.inf
                else:
                    res["status"][s], res["lower_bound"][s] = 2, tree.bound(self.fix[s])
                continue
            self._search(tree, s, res, dive=first_pass and tree.dive_first)
        if hit is not None and (self.inject == "status4" or self.log["injected_returns"] >= 2):   # the pass in which solve_handoff drops the node
            others = [s for s in np.flatnonzero(self.inst == self.inst[hit]) if s != hit and res["status"][s] == 2]
            self.log["dropped_beside_open"] += 1 if others else 0
        if first_pass:
            self.log["first_status"] = res["status"].copy()
        self.res = res
        return dict(solve_ms=0.0)

    def download(self):
        return {k: self.res[k].copy() for k in ("v", "obj", "status", "lower_bound", "nodes", "pivots")}

    def open_nodes(self):
        if not self.recording:
            raise MldGpuError("open nodes were not recorded")
        return tuple(self.res[k].copy() for k in ("depth", "var", "val", "flag"))

    # -- one search -----------------------------------------------------------------------------
    def _search(self, tree, s, res, dive):
        fix, limit = self.fix[s], int(self.opts.max_nodes)
        gap_abs, gap_rel = float(self.opts.gap_abs), float(self.opts.gap_rel)
        st = dict(best=float(self.cut[s]), count=0, inc=None)
        tol = lambda: max(gap_abs, gap_rel * abs(st["best"])) if np.isfinite(st["best"]) else 0.0
        closes = lambda a: not (tree.bound(a) < st["best"] - tol())         # nothing in the node beats the incumbent / cutoff by the gap
        if dive and not np.isfinite(st["best"]):
            # a search that has not become a complete depth-first search yet (dive, deepening passes): a point from a heuristic, no stack
            cand = np.flatnonzero(tree.mask(fix) & np.isfinite(tree.leaf))
            k = int(cand[tree.branch_rng(fix).integers(cand.size)])
            res["obj"][s], res["v"][s, 0], res["v"][s, 1:] = tree.leaf[k], tree.leaf[k], tree.bits[k]
            res["status"][s], res["lower_bound"][s], res["nodes"][s], res["pivots"][s] = 2, min(tree.bound(fix), tree.leaf[k]), limit, 7 * limit
            return

        def enter(a):
            if st["count"] >= limit:
                return "stop"
            st["count"] += 1
            return "prune" if closes(a) else None

        def choose(a, rest):
            rng = tree.branch_rng(a)
            j, first = rest[int(rng.integers(len(rest)))], int(rng.integers(0, 2))
            sib = a.copy(); sib[j] = 1 - first
            return j, first, bool(rng.random() < 0.2) and closes(sib)

        def leaf(a):
            st["best"], st["inc"] = tree.bound(a), a.copy()                 # entered, so it beats the incumbent by more than the gap

        stack = stack_dfs(fix, enter, choose, leaf)
        res["nodes"][s], res["pivots"][s] = st["count"], 7 * st["count"]
        if st["inc"] is not None:
            res["obj"][s], res["v"][s, 0], res["v"][s, 1:] = st["best"], st["best"], st["inc"]
        closed_at = st["best"] - tol() if np.isfinite(st["best"]) else np.inf   # every closed node's bound is at least this
        if stack is None:
            res["status"][s] = 0 if st["inc"] is not None else 1
            res["lower_bound"][s] = st["best"] if st["inc"] is not None else closed_at
            return
        res["status"][s], res["depth"][s] = 2, len(stack)
        for k, (j, val, flag) in enumerate(stack):
            res["var"][s, k], res["val"][s, k], res["flag"][s, k] = j + 1, val, flag    # the decision vector's index: entry 0 is continuous
        pos = np.full(self.n, -1, np.int64)
        pos[1:] = np.arange(self.n_bin)
        open_ = gpu.expand_open_nodes(fix, len(stack), res["var"][s], res["val"][s], res["flag"][s], pos)
        res["lower_bound"][s] = min(min(tree.bound(f) for f in open_), closed_at)
