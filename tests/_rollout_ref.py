"""Helpers of the rollout tests (tests/test_rollout_host.py, tests/test_gpu_rollout.py): the closed form of tests/_aux_ref.py as the resolve_fn of
simlog.rollout_np, and a library of S realised series per instance.  CPU only."""
import numpy as np

import _aux_ref
from pyhybridcontrol_amd import profiles


def closed_form_resolver(mats_list, d):
    """resolve_fn(x, u, omega, model_idx) -> dict(v = [delta | z | mu], status): the closed form per instance's model.  On the hard variant (nmu = 0) a tank
    outside its bounds leaves no feasible point: status 1 and a NaN row, as the resolver returns it."""
    nmu = int(d.get("nmu", 0))

    def fn(x, u, om, midx):
        n = np.shape(x)[0]
        v, status = np.zeros((n, 2 + nmu)), np.zeros(n, np.int32)
        for k, mats in enumerate(mats_list):
            sel = np.asarray(midx) == k
            if not sel.any():
                continue
            cf = _aux_ref.closed_form(mats, d, x[sel], u[sel], om[sel])
            if nmu:
                v[sel] = cf["v"]
            else:
                v[sel] = np.hstack([cf["delta"], cf["z"]])
                bad = cf["mu"].max(axis=1) > 0
                rows = np.where(sel)[0][bad]
                v[rows], status[rows] = np.nan, 1
        return dict(v=v, status=status)
    return fn


def closed_y(mats_list, d, midx, u_seq, omega_seq):
    """the closed form's y = D1 u + omega_load of every step of every trajectory, (B, S, K): the guard |y| >= 1e-3 keeps every instance off the switching surface"""
    D1 = np.stack([np.asarray(m["D1"], float).reshape(-1) for m in mats_list])[np.asarray(midx)]
    return np.einsum("bkj,bj->bk", u_seq, D1)[:, None, :] + omega_seq[..., d["nx"]]


def realised_library(om, N, nw, nx, S, K, step, rng, sigma=800.0):
    """per instance and realisation two series (groups of widths 1 and nomega - 1): the forecast tiled, its load channel moved by N(0, sigma)
    (without a load channel, nomega == nx: every channel scaled by 1 + N(0, 0.2)).
    Returns (lib, group widths, start (B, S, 2), omega_seq (B, S, K, nomega) = the windows of K steps from `step`)."""
    B = om.shape[0]
    gw = (1, nw - 1)
    T = K + step + 1
    series = []
    for b in range(B):
        for _ in range(S):
            s = np.tile(om[b].reshape(N, nw), (T // N + 1, 1))[:T].copy()
            if nx < nw:
                s[:, nx] += rng.normal(0.0, sigma, T)
            else:                                                        # (a model without the load channel: every draw moved by a fifth)
                s *= 1.0 + 0.2 * rng.standard_normal(s.shape)
            series += [s[:, :1], s[:, 1:]]
    lib, base = profiles.pack(series)
    start = np.asarray(base, np.int64).reshape(B, S, 2)
    return lib, gw, start, profiles.windows(lib, start, step, K, gw).reshape(B, S, K, nw)
