extern "C" {

// ---- RCCL gather ---------------------------------------------------------------------------------
static ncclComm_t g_comm = nullptr;
static int g_nranks = 0;

int mld_comm_unique_id(uint8_t id[MLD_COMM_ID_BYTES])
{
    static_assert(sizeof(ncclUniqueId) <= MLD_COMM_ID_BYTES, "id size");
    ncclUniqueId u;
    ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) { mld_set_error("ncclGetUniqueId: %s", ncclGetErrorString(r)); return MLD_ERR_COMM; }
    memset(id, 0, MLD_COMM_ID_BYTES);
    memcpy(id, &u, sizeof(u));
    return MLD_OK;
}

int mld_comm_init(int n_ranks, int rank, const uint8_t id[MLD_COMM_ID_BYTES])
{
    if (mld_device_count() <= 0) { mld_set_error("no HIP device"); return MLD_ERR_NO_DEVICE; }
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclResult_t r = ncclCommInitRank(&g_comm, n_ranks, u, rank);
    if (r != ncclSuccess) { mld_set_error("ncclCommInitRank: %s", ncclGetErrorString(r)); return MLD_ERR_COMM; }
    g_nranks = n_ranks;
    return MLD_OK;
}

int mld_gather(const double *send, int count, double *recv)
{
    if (!g_comm) { mld_set_error("mld_gather: communicator not initialised"); return MLD_ERR_COMM; }
    DevBuf<double> d_s, d_r;
    HIP_TRY(d_s.alloc(std::max(1, count)));
    HIP_TRY(d_r.alloc((size_t)std::max(1, count) * g_nranks));
    hipError_t e = hipMemcpy(d_s, send, sizeof(double) * count, hipMemcpyHostToDevice);
    ncclResult_t r = ncclSuccess;
    if (e == hipSuccess) r = ncclAllGather(d_s, d_r, count, ncclDouble, g_comm, 0);
    if (e == hipSuccess && r == ncclSuccess) e = hipStreamSynchronize(0);
    if (e == hipSuccess && r == ncclSuccess) e = hipMemcpy(recv, d_r, sizeof(double) * count * g_nranks, hipMemcpyDeviceToHost);
    if (r != ncclSuccess) { mld_set_error("ncclAllGather: %s", ncclGetErrorString(r)); return MLD_ERR_COMM; }
    if (e != hipSuccess) { mld_set_error("mld_gather: %s", hipGetErrorString(e)); return MLD_ERR_HIP; }
    return MLD_OK;
}

} // extern "C"

extern "C" int mld_gather_results(mld_problem_t *p, double *recv, int *width_out)
{
    if (!g_comm) { mld_set_error("mld_gather_results: communicator not initialised"); return MLD_ERR_COMM; }
    if (!p || p->batch < 1 || !recv) { mld_set_error("mld_gather_results: nothing solved"); return MLD_ERR_INVALID; }
    if (int rc = entry_guard(p, "mld_gather_results", false, nullptr)) return rc;
    const int w = 2 + p->nv;
    const size_t count = (size_t)p->batch * w;
    /* send / receive buffers live with the problem (a hipFree per call synchronises the whole device: with two handles in flight the gather of
     * one would wait for the other's solve), and pack + all-gather run on the problem's own stream */
    if (p->gather_cap < count * (size_t)(1 + g_nranks)) {
        p->gather_cap = 0;
        HIP_TRY(p->d_gather.alloc(count * (size_t)(1 + g_nranks)));
        p->gather_cap = count * (size_t)(1 + g_nranks);
    }
    double *d_s = p->d_gather, *d_r = p->d_gather + count;
    const hipStream_t sq = p->stream;
    hipLaunchKernelGGL(k_pack_results, dim3((unsigned)std::min<size_t>((count + 255) / 256, 65535)), dim3(256), 0, sq, p->batch, p->n, p->nv, p->bat.obj, p->bat.status, p->bat.v, d_s);
    hipError_t e = hipGetLastError();
    ncclResult_t r = e == hipSuccess ? ncclAllGather(d_s, d_r, count, ncclDouble, g_comm, sq) : ncclSuccess;
    if (r == ncclSuccess && e == hipSuccess) e = hipMemcpyAsync(recv, d_r, sizeof(double) * count * g_nranks, hipMemcpyDeviceToHost, sq);
    if (r == ncclSuccess && e == hipSuccess) e = hipStreamSynchronize(sq);
    if (r != ncclSuccess) { mld_set_error("ncclAllGather: %s", ncclGetErrorString(r)); return MLD_ERR_COMM; }
    if (e != hipSuccess) { mld_set_error("mld_gather_results: %s", hipGetErrorString(e)); return MLD_ERR_HIP; }
    if (width_out) *width_out = w;
    return MLD_OK;
}

extern "C" int mld_comm_destroy(void)
{
    if (g_comm) { ncclCommDestroy(g_comm); g_comm = nullptr; }
    return MLD_OK;
}
