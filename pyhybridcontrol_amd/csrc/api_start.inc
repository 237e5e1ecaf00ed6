// MIP start from a rollout of the resident forecast (mld_warm_start_from_rollout): the route from the rollout kernels to the start buffer, on the device.
// The rollout is rollout_impl's (api_rollout.inc) with a StartCall -- K = N_tilde, S = 1, the disturbance the resident forecast, v and end_status device
// temporaries --, the start k_warm_from_rollout's (kernels.inc, the byte rule in warm_rollout.inc).  Every check is rollout_impl's own.
extern "C" {

int mld_warm_start_from_rollout(mld_problem_t *p, mld_problem_t *aux, int policy, const double *u_seq, const double *u_prev, int flags, int32_t *source_out,
                                int64_t stats[4])
{
    static const char who[] = "mld_warm_start_from_rollout";
    if (int rc = entry_guard(p, who, true, "no batch resident (mld_upload_batch)")) return rc;
    if (policy != 0 && policy != 1) { mld_set_error("%s: policy = %d (0 = the caller's u_seq through k_rollout, 1 = the resident policy through k_rollout_policy)", who, policy); return MLD_ERR_INVALID; }
    if (flags & ~MLD_START_KEEP) { mld_set_error("%s: unknown flag bits 0x%x (MLD_START_KEEP = 1 is the only one)", who, (unsigned)(flags & ~MLD_START_KEEP)); return MLD_ERR_INVALID; }
    if (!policy && !u_seq) { mld_set_error("%s: policy = 0 needs u_seq (batch, N_tilde, nu) -- a start from the handle's own resident plan is mld_warm_start_from_previous", who); return MLD_ERR_INVALID; }
    if (!policy && u_prev) { mld_set_error("%s: u_prev given with policy = 0 (the open-loop rollout has no previous input)", who); return MLD_ERR_INVALID; }
    const StartCall sc{(flags & MLD_START_KEEP) != 0, source_out, stats};
    const PolicyCall pc{u_prev, nullptr};
    const RolloutOut none{};      /* nothing of the rollout comes back to the host: v and end_status feed k_warm_from_rollout on the device */
    return rollout_impl(who, policy ? &pc : nullptr, p, aux, /* K */ p->N, /* S */ 1, u_seq, /* omega_seq */ nullptr, /* start */ nullptr, /* step */ 0,
                        /* cost_w */ nullptr, /* cost_rows */ 0, none, &sc);
}

} // extern "C"
