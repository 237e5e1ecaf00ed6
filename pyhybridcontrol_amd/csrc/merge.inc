// ---- in-kernel hand-off: merging the items of a tree into its root instance (after k_solve, same stream) ----
/* (C linkage, as they have always had: the names are part of the code object and of the library's symbol list) */
extern "C" {
// order-preserving map double -> unsigned 64 (atomicMin on it = minimum of the doubles)
__device__ __forceinline__ unsigned long long mg_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double mg_val(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ bool mg_unclosed(int st) { return st == MLD_STATUS_NODE_LIMIT || st == MLD_STATUS_NUMERICAL || st == MLD_STATUS_EXPANDED_OPEN; }

__global__ void __launch_bounds__(256) k_merge_init(int batch, const double *obj, unsigned long long *best, unsigned long long *lbopen, unsigned long long *label, int *open_cnt)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= batch) return;
    best[r] = mg_key(obj[r]); lbopen[r] = mg_key(__builtin_huge_val()); label[r] = ~0ull; open_cnt[r] = 0;
}
// pass A: every item adds itself to its root -- best objective, what it left open, work counters
__global__ void __launch_bounds__(256) k_merge_a(int batch, const int *tail, const int *root, const double *obj, const double *lb, const int *status,
                                                 int *nodes, int *pivots, int *cuts, int *refac, long long *rows,
                                                 unsigned long long *best, unsigned long long *lbopen, int *open_cnt, const int *dead)
{
    const int it = batch + blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= *tail) return;
    const int r = root[it];
    if (dead[r]) return;              // a tree that was given up keeps its root's own result
    atomicMin(&best[r], mg_key(obj[it]));
    if (mg_unclosed(status[it])) { atomicAdd(&open_cnt[r], 1); atomicMin(&lbopen[r], mg_key(lb[it])); }
    atomicAdd(&nodes[r], nodes[it]); atomicAdd(&pivots[r], pivots[it]); atomicAdd(&cuts[r], cuts[it]); atomicAdd(&refac[r], refac[it]);
    atomicAdd((unsigned long long *)&rows[r], (unsigned long long)rows[it]);
}
// pass B: among the entries that hold the best objective the smallest tree label wins (deterministic whatever the queue order was)
__global__ void __launch_bounds__(256) k_merge_b(int batch, const int *tail, const int *root, const double *obj, const long long *lab,
                                                 const unsigned long long *best, unsigned long long *label, const int *dead)
{
    const int it = batch + blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= *tail) return;
    const int r = root[it];
    if (dead[r]) return;
    if (mg_key(obj[it]) == best[r] && obj[it] < 1.0e300) atomicMin(&label[r], (unsigned long long)lab[it]);
}
// pass C: the winning item's point becomes the root's (one workgroup per item; the root's own point stays when its objective is the best)
__global__ void __launch_bounds__(256) k_merge_c(int batch, const int *tail, int n, const int *root, const double *obj, const long long *lab,
                                                 const unsigned long long *best, const unsigned long long *label, double *v, const int *dead)
{
    const int it = batch + blockIdx.x;
    if (it >= *tail) return;
    const int r = root[it];
    if (dead[r]) return;
    if (mg_key(obj[it]) != best[r] || !(obj[it] < 1.0e300) || (unsigned long long)lab[it] != label[r]) return;
    if (mg_key(obj[r]) == best[r]) return;       // (the root found the same value itself: label 1 is the smallest)
    for (int j = threadIdx.x; j < n; j += blockDim.x) v[(size_t)r * n + j] = v[(size_t)it * n + j];
}
// pass D: status, objective and bound of every root that was split
__global__ void __launch_bounds__(256) k_merge_d(int batch, double gap_abs, double gap_rel, double *obj, double *lb, int *status,
                                                 const unsigned long long *best, const unsigned long long *lbopen, const int *open_cnt, int *n_unfinished, const int *dead, int *n_dead)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= batch) return;
    if (dead[r]) {                   // given up: the root's own incumbent and bound, as it stopped
        if (status[r] == MLD_STATUS_EXPANDED || status[r] == MLD_STATUS_EXPANDED_OPEN) status[r] = MLD_STATUS_NODE_LIMIT;
        atomicAdd(n_unfinished, 1); atomicAdd(n_dead, dead[r] == 2 ? 65536 : 1);
        return;
    }
    if (status[r] != MLD_STATUS_EXPANDED && status[r] != MLD_STATUS_EXPANDED_OPEN) return;
    const bool own_open = status[r] == MLD_STATUS_EXPANDED_OPEN;
    const double o = mg_val(best[r]);
    const bool fin = o < 1.0e300;
    const double tol = fin ? fmax(gap_abs, gap_rel * fabs(o)) : 0.0;
    obj[r] = o;
    if (open_cnt[r] == 0 && !own_open) {       // every node of the tree is closed: proven
        status[r] = fin ? MLD_STATUS_OPTIMAL : MLD_STATUS_INFEASIBLE;
        if (fin) lb[r] = fmin(o, fmax(lb[r], o - tol));
    } else {
        status[r] = MLD_STATUS_NODE_LIMIT;
        lb[r] = own_open ? fmin(lb[r], fin ? o : __builtin_huge_val())      /* (the root's own rest is open: its bound, valid for the whole tree, stands) */
                         : fmax(lb[r], fmin(mg_val(lbopen[r]), fin ? o - tol : __builtin_huge_val()));
        atomicAdd(n_unfinished, 1);
    }
}
}

/* an empty hand-off queue behind the batch's instances (before k_solve) */
static int handoff_reset(mld_problem *p)
{
    const hipStream_t sq = p->stream;
    const int batch = p->batch;
    const BatchBufs::Handoff &q = p->bat.ho;
    HIP_TRY(hipMemsetAsync(q.tree_count, 0, sizeof(int) * (size_t)batch * 9, sq));
    HIP_TRY(hipMemsetAsync(q.tree_dead, 0, sizeof(int) * (size_t)batch, sq));
    hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, sq, q.tail, batch);
    HIP_TRY(hipMemsetAsync(q.finished, 0, sizeof(int), sq));
    HIP_TRY(hipMemsetAsync(q.item_ready, 0, sizeof(int) * (size_t)p->batch_cap, sq));
    HIP_TRY(hipMemsetAsync(q.item_children, 0, sizeof(int) * (size_t)p->batch_cap, sq));
    if (!p->has_cutoff) hipLaunchKernelGGL(k_fill_f64, dim3((batch + 255) / 256), dim3(256), 0, sq, (size_t)batch, (double)INFINITY, p->bat.cutoff);
    return MLD_OK;
}

/* what the merge works on: the per-entry result arrays (cap entries: batch roots, then the items), the items' roots and tree labels, the
 * give-up marks and the accumulators per root, and the two device counters it reports through.  The solve path fills it from the resident batch
 * (merge_args), mld_debug_merge from arrays of the caller's. */
struct MergeArgs {
    int batch, cap, n; double gap_abs, gap_rel;
    double *obj, *lbnd, *v; int *status, *nodes, *pivots, *cuts, *refac; long long *rows;
    const int *tail, *item_root; const long long *item_label; const int *tree_dead;
    unsigned long long *mg_best, *mg_lbopen, *mg_label; int *mg_open;
    int *n_unfinished, *n_dead;      /* n_dead: + 1 per tree given up for its size, + 65536 per tree given up because the queue was full */
};

static MergeArgs merge_args(const mld_problem *p)
{
    const BatchBufs &b = p->bat;
    const BatchBufs::Handoff &q = b.ho;
    MergeArgs a;
    a.batch = p->batch; a.cap = p->batch_cap; a.n = p->n; a.gap_abs = p->opts.gap_abs; a.gap_rel = p->opts.gap_rel;
    a.obj = b.obj; a.lbnd = b.lbnd; a.v = b.v; a.status = b.status; a.nodes = b.nodes; a.pivots = b.pivots; a.cuts = b.cuts; a.refac = b.refac; a.rows = b.rows;
    a.tail = q.tail; a.item_root = q.item_root; a.item_label = q.item_label; a.tree_dead = q.tree_dead;
    a.mg_best = q.mg_best; a.mg_lbopen = q.mg_lbopen; a.mg_label = q.mg_label; a.mg_open = q.mg_open;
    a.n_unfinished = b.skipped; a.n_dead = q.finished;      /* (finished: the queue is drained, the counter is free) */
    return a;
}

/* merge the items into their roots after k_solve (deterministic: best objective, smallest tree label on ties) */
static int handoff_merge(const MergeArgs &a, hipStream_t sq)
{
    const int batch = a.batch;
    const int items = a.cap - batch;
    const dim3 gi((items + 255) / 256), gb((batch + 255) / 256), blk(256);
    HIP_TRY(hipMemsetAsync(a.n_unfinished, 0, sizeof(int), sq));
    hipLaunchKernelGGL(k_merge_init, gb, blk, 0, sq, batch, a.obj, a.mg_best, a.mg_lbopen, a.mg_label, a.mg_open);
    hipLaunchKernelGGL(k_merge_a, gi, blk, 0, sq, batch, a.tail, a.item_root, a.obj, a.lbnd, a.status, a.nodes, a.pivots, a.cuts, a.refac, a.rows,
                       a.mg_best, a.mg_lbopen, a.mg_open, a.tree_dead);
    hipLaunchKernelGGL(k_merge_b, gi, blk, 0, sq, batch, a.tail, a.item_root, a.obj, a.item_label, a.mg_best, a.mg_label, a.tree_dead);
    hipLaunchKernelGGL(k_merge_c, dim3(items), blk, 0, sq, batch, a.tail, a.n, a.item_root, a.obj, a.item_label, a.mg_best, a.mg_label, a.v, a.tree_dead);
    hipLaunchKernelGGL(k_merge_d, gb, blk, 0, sq, batch, a.gap_abs, a.gap_rel, a.obj, a.lbnd, a.status, a.mg_best, a.mg_lbopen, a.mg_open, a.n_unfinished, a.tree_dead, a.n_dead);
    return MLD_OK;
}

extern "C" {

/* The hand-off merge on a queue of the caller's (internal diagnostics and tests; not part of the public header): per-entry arrays of `cap` entries -- `batch`
 * roots, then items up to `tail` -- are uploaded, handoff_merge runs on them exactly as after k_solve, and the roots' results come back in place
 * (obj, lbnd, status, nodes, pivots, cuts, refac, rows: entries < batch; v: rows < batch of cap x n).  item_root / item_label: cap entries, read in
 * [batch, tail); tree_dead: batch entries (0, 1 = given up for its size, 2 = for a full queue).  n_unfinished, finished: the two device counters, finished
 * starting at tail as a drained queue leaves it.  Everything a kernel indexes with is validated here. */
struct mld_debug_merge_io {
    int32_t batch, cap, n, tail; double gap_abs, gap_rel;
    double *obj, *lbnd, *v; int32_t *status, *nodes, *pivots, *cuts, *refac; int64_t *rows;
    const int32_t *item_root; const int64_t *item_label; const int32_t *tree_dead;
    int32_t n_unfinished, finished;
};
int mld_debug_merge(mld_debug_merge_io *io)
{
    if (!io || !io->obj || !io->lbnd || !io->v || !io->status || !io->nodes || !io->pivots || !io->cuts || !io->refac || !io->rows || !io->item_root ||
        !io->item_label || !io->tree_dead) { mld_set_error("mld_debug_merge: null argument"); return MLD_ERR_INVALID; }
    const int batch = io->batch, cap = io->cap, n = io->n, tail = io->tail;
    if (batch < 1 || cap <= batch || tail < batch || tail > cap || n < 1 || (size_t)cap * (size_t)n > ((size_t)1 << 28)) {
        mld_set_error("mld_debug_merge: need 1 <= batch <= tail <= cap, cap > batch, n >= 1 (batch %d, tail %d, cap %d, n %d)", batch, tail, cap, n); return MLD_ERR_INVALID;
    }
    if (!(io->gap_abs >= 0.0) || !(io->gap_rel >= 0.0)) { mld_set_error("mld_debug_merge: gaps must be >= 0"); return MLD_ERR_INVALID; }
    for (int it = batch; it < tail; ++it) if (io->item_root[it] < 0 || io->item_root[it] >= batch) { mld_set_error("mld_debug_merge: item_root[%d] = %d is no root", it, io->item_root[it]); return MLD_ERR_INVALID; }
    for (int r = 0; r < batch; ++r) if (io->tree_dead[r] < 0 || io->tree_dead[r] > 2) { mld_set_error("mld_debug_merge: tree_dead[%d] = %d", r, io->tree_dead[r]); return MLD_ERR_INVALID; }
    const size_t c = cap, b = batch;
    DevBuf<double> obj, lbnd, v; DevBuf<int> status, nodes, pivots, cuts, refac, item_root, tree_dead, tl, unf, fin, mg_open;
    DevBuf<long long> rows, item_label; DevBuf<unsigned long long> mg_best, mg_lbopen, mg_label;
    HIP_TRY(obj.alloc(c)); HIP_TRY(lbnd.alloc(c)); HIP_TRY(v.alloc(c * n)); HIP_TRY(status.alloc(c)); HIP_TRY(nodes.alloc(c)); HIP_TRY(pivots.alloc(c));
    HIP_TRY(cuts.alloc(c)); HIP_TRY(refac.alloc(c)); HIP_TRY(rows.alloc(c)); HIP_TRY(item_root.alloc(c)); HIP_TRY(item_label.alloc(c)); HIP_TRY(tree_dead.alloc(b));
    HIP_TRY(tl.alloc(1)); HIP_TRY(unf.alloc(1)); HIP_TRY(fin.alloc(1));
    HIP_TRY(mg_best.alloc(b)); HIP_TRY(mg_lbopen.alloc(b)); HIP_TRY(mg_label.alloc(b)); HIP_TRY(mg_open.alloc(b));
    HIP_TRY(hipMemcpy(obj, io->obj, sizeof(double) * c, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(lbnd, io->lbnd, sizeof(double) * c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v, io->v, sizeof(double) * c * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(status, io->status, sizeof(int) * c, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(nodes, io->nodes, sizeof(int) * c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pivots, io->pivots, sizeof(int) * c, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(cuts, io->cuts, sizeof(int) * c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(refac, io->refac, sizeof(int) * c, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(rows, io->rows, sizeof(long long) * c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(item_root, io->item_root, sizeof(int) * c, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(item_label, io->item_label, sizeof(long long) * c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(tree_dead, io->tree_dead, sizeof(int) * b, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(tl, &tail, sizeof(int), hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(fin, &tail, sizeof(int), hipMemcpyHostToDevice));
    MergeArgs a;
    a.batch = batch; a.cap = cap; a.n = n; a.gap_abs = io->gap_abs; a.gap_rel = io->gap_rel;
    a.obj = obj; a.lbnd = lbnd; a.v = v; a.status = status; a.nodes = nodes; a.pivots = pivots; a.cuts = cuts; a.refac = refac; a.rows = rows;
    a.tail = tl; a.item_root = item_root; a.item_label = item_label; a.tree_dead = tree_dead;
    a.mg_best = mg_best; a.mg_lbopen = mg_lbopen; a.mg_label = mg_label; a.mg_open = mg_open; a.n_unfinished = unf; a.n_dead = fin;
    if (int rc = handoff_merge(a, 0)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(io->obj, obj, sizeof(double) * b, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(io->lbnd, lbnd, sizeof(double) * b, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(io->v, v, sizeof(double) * b * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(io->status, status, sizeof(int) * b, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(io->nodes, nodes, sizeof(int) * b, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(io->pivots, pivots, sizeof(int) * b, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(io->cuts, cuts, sizeof(int) * b, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(io->refac, refac, sizeof(int) * b, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(io->rows, rows, sizeof(long long) * b, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&io->n_unfinished, unf, sizeof(int), hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(&io->finished, fin, sizeof(int), hipMemcpyDeviceToHost));
    return MLD_OK;
}

} // extern "C"
