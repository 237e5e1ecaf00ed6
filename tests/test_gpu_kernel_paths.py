"""Parity of every dispatch branch of the kernels that build the solver's input -- condensing (K1/K2), constraint right-hand
sides (K3) and cost pull-back (K4) -- against plain fp64 numpy restatements of the same operation: condense_np.condense /
condense_tv, h = H_x x + H_w w + H_5 (row-min over scenarios) and _paths.ref_cost.  Each case names the kernel or template
instantiation it targets and the condition that sends it there (csrc/condense.inc condense_model_device, csrc/api_solve.inc
mld_rhs_batch / csrc/api_create.inc set_cost_impl).  Random models come from _paths.random_mld (fixed seeds, spectral radius of A in [0.9, 1.05])."""
import numpy as np
import pytest

import _paths
import _tv
import condense_np as cn
from pyhybridcontrol_amd import gpu, synthetic as syn, _lib

pytestmark = pytest.mark.gpu

EVO = _paths.EVO_NAMES
TINY = dict(nx=2, nu=1, nomega=1, ny=1, nc=2)                                   # 512 of them stay cheap
MID = dict(nx=5, nu=2, ndelta=1, nz=1, nmu=2, nomega=3, ny=2, nc=6)


def _models(n, seed, **dims):
    out = [_paths.random_mld(seed * 100000 + i, **dims) for i in range(n)]
    return [m for m, _, _ in out], out[0][1]


def _check_evo(evo, refs, tol=1e-11):
    """all 12 maps of every model within tol x max(1, |ref|) per map"""
    for i, ref in enumerate(refs):
        for nm in EVO:
            r, g = ref[nm], evo[nm][i]
            assert g.shape == r.shape, (i, nm, g.shape, r.shape)
            if r.size:
                err = float(np.abs(g - r).max())
                assert err <= tol * max(1.0, float(np.abs(r).max())), (i, nm, err)


def _condense_and_check(mats_list, dims, N, dtype=np.float64):
    m = gpu.GpuModel(mats_list, dims)
    try:
        evo = m.condense(N)
        _check_evo(evo, [cn.condense(a, N) for a in mats_list])
        if dtype == np.float32:
            e32 = m.condense(N, dtype=np.float32)
            for nm in EVO:
                assert e32[nm].dtype == np.float32 and np.array_equal(e32[nm], evo[nm].astype(np.float32)), nm
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- K1 / K2
@pytest.mark.parametrize("n_models", [16, 64, 256, 512])
def test_condense_model_natural_split(n_models, monkeypatch):
    """k_condense_model without overrides: split = the smallest power of two with n_models * split >= 512, capped at N = 25
    -> 25 (capped, 256 threads), 8 (256), 2 (512 threads) and 1 (1024 threads); with split < N a workgroup owns
    nk = ceil((N - k0) / split) blocks and the nkm-sized LDS arrays hold several of them"""
    monkeypatch.delenv("MLD_K1_SPLIT", raising=False)
    monkeypatch.delenv("MLD_K1_PER_BLOCK", raising=False)
    mats, d = _models(n_models, 1, **TINY)
    _condense_and_check(mats, d, 25)


@pytest.mark.parametrize("split", [1, 2, 3, 7, 24, 25, 31])
def test_condense_model_forced_split(split, monkeypatch):
    """k_condense_model with MLD_K1_SPLIT: uneven dealing of the 25 blocks (3, 7, 24), one block per workgroup (25), idle
    workgroups k0 >= N (31), and the 1024 / 512-thread launches (1, 2)"""
    monkeypatch.setenv("MLD_K1_SPLIT", str(split))
    monkeypatch.delenv("MLD_K1_PER_BLOCK", raising=False)
    mats, d = _models(3, 2, **MID)
    _condense_and_check(mats, d, 25)


@pytest.mark.parametrize("split", [None, 1, 2])
@pytest.mark.parametrize("N", [1, 2])
def test_condense_model_degenerate_horizons(N, split, monkeypatch):
    """k_condense_model at N = 1 (no prefix doubling, Pw[1] never written) and N = 2, natural split and forced"""
    if split is None:
        monkeypatch.delenv("MLD_K1_SPLIT", raising=False)
    else:
        monkeypatch.setenv("MLD_K1_SPLIT", str(split))
    mats, d = _models(3, 3, **MID)
    _condense_and_check(mats, d, N)


def test_condense_blocks_automatic_fallback(monkeypatch):
    """k_condense_blocks reached without MLD_K1_PER_BLOCK: a cfg5-sized model (nx = 15, N = 49) with MLD_K1_SPLIT = 1 needs
    lds_model > 144 KB, so condense_model_device falls back to the per-block kernel"""
    monkeypatch.setenv("MLD_K1_SPLIT", "1")
    monkeypatch.delenv("MLD_K1_PER_BLOCK", raising=False)
    mats, d = _models(1, 4, nx=15, nu=15, ndelta=1, nz=1, nmu=30, nomega=16, ny=1, nc=36)
    _condense_and_check(mats, d, 49)


def test_condense_blocks_above_64k_lds(monkeypatch):
    """k_condense_blocks (MLD_K1_PER_BLOCK) with 83 KB of dynamic LDS: nothing but the block sizes bounds its launch"""
    monkeypatch.setenv("MLD_K1_PER_BLOCK", "1")
    mats, d = _models(2, 6, nx=16, nu=40, ndelta=10, nz=5, nmu=5, nomega=8, ny=2, nc=80)
    _condense_and_check(mats, d, 4)


def test_condense_flat_fp32_on_multi_block_layout(monkeypatch):
    """k_condense_flat<float> after k_condense_model with split = 8 (64 models): every element bit-equal to the fp64 result
    rounded once to fp32"""
    monkeypatch.delenv("MLD_K1_SPLIT", raising=False)
    monkeypatch.delenv("MLD_K1_PER_BLOCK", raising=False)
    mats, d = _models(64, 5, **TINY)
    _condense_and_check(mats, d, 25, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------- time-varying
def _tv_check(horizons, dims, N):
    m = gpu.GpuModel(horizons, dims, time_varying=True)
    try:
        evo = m.condense(N)
        _check_evo(evo, [cn.condense_tv(h) for h in horizons])
    finally:
        m.close()


def test_tv_rows_large_instantiation_by_nx(monkeypatch):
    """k_tv_chain + k_tv_rows<16, 16, 2>: the tank cluster with n_h = 9 has nx = 9 > 8 (and wmax = 25 * 29 = 725)"""
    monkeypatch.delenv("MLD_TV_CHAIN_ONLY", raising=False)
    mats, d, _ = syn.make_agent(9, np.random.default_rng(9), tie=True)
    N = 25
    horizons = [_tv.step_models(mats, N, seed=30 + i, strength=0.2) for i in range(2)]
    _tv_check(horizons, d, N)


def test_tv_rows_large_instantiation_by_width(monkeypatch):
    """k_tv_rows<16, 16, 2> with nx = 4 <= 8: wmax = N max(nv, nw) = 30 * 25 = 750 is above the 640 columns of <8, 10, 4>"""
    monkeypatch.delenv("MLD_TV_CHAIN_ONLY", raising=False)
    horizons = [_paths.random_horizon(40 + i, 30, nx=4, nu=20, nz=3, nmu=2, nomega=4, ny=2, nc=6)[0] for i in range(2)]
    _tv_check(horizons, _paths.make_dims(nx=4, nu=20, nz=3, nmu=2, nomega=4, ny=2, nc=6), 30)


def test_tv_single_kernel_by_nx(monkeypatch):
    """k_condense_tv without MLD_TV_CHAIN_ONLY: nx = 17 > 16 rules the wide path out"""
    monkeypatch.delenv("MLD_TV_CHAIN_ONLY", raising=False)
    dims = dict(nx=17, nu=3, ndelta=1, nomega=2, ny=2, nc=5)
    horizons = [_paths.random_horizon(50 + i, 12, **dims)[0] for i in range(2)]
    _tv_check(horizons, _paths.make_dims(**dims), 12)


def test_tv_wide_path_needs_the_chain_to_fit_lds(monkeypatch):
    """nx = 16, N = 48, one input: k_tv_rows fits (112 KB) but k_tv_chain's N nx^2 + N nx + 32 nx^2 doubles (166 KB) do not;
    the shape must go to k_condense_tv.  (Was wrong: the wide path was chosen on k_tv_rows' LDS alone, k_tv_chain's launch
    failed and condensing returned MLD_ERR_HIP for a shape k_condense_tv handles.)"""
    monkeypatch.delenv("MLD_TV_CHAIN_ONLY", raising=False)
    dims = dict(nx=16, nu=1, nomega=1, ny=1, nc=2)
    horizons = [_paths.random_horizon(55, 48, **dims)[0]]
    _tv_check(horizons, _paths.make_dims(**dims), 48)


def test_tv_single_kernel_lds_limit_is_an_error(monkeypatch):
    """k_condense_tv's LDS (3 nx^2 + 9 nx (nv + nw) + ... doubles) above 150 KB: MLD_ERR_UNSUPPORTED, never numbers"""
    monkeypatch.delenv("MLD_TV_CHAIN_ONLY", raising=False)
    dims = dict(nx=40, nu=40, nomega=10, ny=4, nc=40)
    horizons = [_paths.random_horizon(60, 3, **dims)[0]]
    m = gpu.GpuModel(horizons, _paths.make_dims(**dims), time_varying=True)
    try:
        with pytest.raises(gpu.MldGpuError):
            m.condense(3)
    finally:
        m.close()


@pytest.mark.parametrize("N", [1, 2])
def test_tv_wide_path_degenerate_horizons(N, monkeypatch):
    """k_tv_chain + k_tv_rows<8, 10, 4> at N = 1 (only the identity chain) and N = 2, three horizons per handle"""
    monkeypatch.delenv("MLD_TV_CHAIN_ONLY", raising=False)
    horizons = [_paths.random_horizon(70 + 10 * N + i, N, **MID)[0] for i in range(3)]
    _tv_check(horizons, _paths.make_dims(**MID), N)


# ------------------------------------------------------------------------------------------------------------------- K3
RHS_PATHS = (("mfma64", dict()), ("valu", dict(reserved=128)), ("mfma32", dict(flags=_lib.MLD_F32)))
# name -> (N, dims); K = nx + N nw, m0 = N nc
RHS_SHAPES = {
    "K40": (12, dict(nx=4, nu=2, ndelta=1, nomega=3, ny=1, nc=5)),        # K = 0 mod 4 (no padding), m0 = 60
    "K41": (12, dict(nx=5, nu=2, ndelta=1, nomega=3, ny=1, nc=4)),        # K = 1 mod 4, m0 = 48
    "K42": (12, dict(nx=6, nu=2, ndelta=1, nomega=3, ny=1, nc=3)),        # K = 2 mod 4
    "K43": (12, dict(nx=7, nu=2, ndelta=1, nomega=3, ny=1, nc=5)),        # K = 3 mod 4
    "K317": (20, dict(nx=17, nu=1, ndelta=1, nomega=15, ny=1, nc=3)),     # Kp = 320 with a padded last fragment
    "K320": (20, dict(nx=20, nu=1, ndelta=1, nomega=15, ny=1, nc=3)),     # Kp = RM_KMAX: all 80 A-fragments live
    "K321": (20, dict(nx=21, nu=1, ndelta=1, nomega=15, ny=1, nc=3)),     # one past RM_KMAX: k_rhs
    "nx0": (10, dict(nx=0, nu=2, ndelta=1, nomega=5, ny=1, nc=4)),        # H_x null
    "nw0": (12, dict(nx=6, nu=2, ndelta=1, nomega=0, ny=1, nc=3)),        # H_w null
    "m0_21": (7, dict(nx=3, nu=1, ndelta=1, nomega=2, ny=1, nc=3)),       # m0 = 21: a partial last 16-row block
}


def _check_rhs(h, ref, s, fp32, K):
    """fp64: within 1e-12 sum_j |H_ij z_j| per row; fp32: within gamma_{K+2} of the same sum (plus the fp64 slack), and not fp64"""
    err = np.abs(h - ref)
    bound = (_paths.fp32_dot_bound(K) + 1e-12) * s if fp32 else 1e-12 * s
    assert np.all(err <= bound), float((err / s).max())
    if fp32:
        assert float((err / s).max()) > 1e-12           # the fp32 kernel really ran


@pytest.mark.parametrize("path", [p for p, _ in RHS_PATHS])
@pytest.mark.parametrize("shape", list(RHS_SHAPES))
def test_rhs_paths(shape, path):
    """K3 through mld_rhs_batch.  rhs_mfma_fits (Kp = (K + 3) & ~3 <= 320) and no opts.reserved bit 7 -> k_rhs_mfma<false>,
    with MLD_F32 k_rhs_mfma<true>; reserved = 128, K = 321 or scenarios > 1 -> k_rhs (fp64).  Per shape: one model with
    model_idx = None (two 128-instance groups), three models interleaved with 170 instances of model 0, 130 of model 2 and
    none of model 1, and three scenarios on the three-model batch (row-min, k_rhs)."""
    N, dims = RHS_SHAPES[shape]
    d = _paths.make_dims(**dims)
    K = d["nx"] + N * d["nomega"]
    kw = dict(RHS_PATHS)[path]
    mfma = path != "valu" and ((K + 3) & ~3) <= 320
    fp32 = path == "mfma32" and mfma
    seed = 1000 + list(RHS_SHAPES).index(shape)
    rng = np.random.default_rng(seed)
    nx, nW = d["nx"], N * d["nomega"]
    # one model, model_idx = None
    mats, _ = _models(1, seed, **dims)
    m = gpu.GpuModel(mats, d)
    p = gpu.GpuProblem(m, N - 1, N, None, **kw)
    try:
        x0, om = rng.standard_normal((150, nx)), rng.standard_normal((150, nW))
        ref, s = _paths.rhs_terms(cn.condense(mats[0], N), x0, om)
        _check_rhs(p.rhs(x0, om), ref, s, fp32, K)
    finally:
        p.close(); m.close()
    # three models, interleaved, model 1 unused
    mats, _ = _models(3, seed + 1, **dims)
    evos = [cn.condense(a, N) for a in mats]
    m = gpu.GpuModel(mats, d)
    p = gpu.GpuProblem(m, N - 1, N, None, **kw)
    try:
        midx = rng.permutation(np.r_[np.zeros(170), np.full(130, 2)]).astype(np.int32)
        x0, om = rng.standard_normal((300, nx)), rng.standard_normal((300, nW))
        ref, s = np.zeros((300, N * d["nc"])), np.zeros((300, N * d["nc"]))
        for k in (0, 2):
            sel = midx == k
            ref[sel], s[sel] = _paths.rhs_terms(evos[k], x0[sel], om[sel])
        _check_rhs(p.rhs(x0, om, midx), ref, s, fp32, K)
        # scenarios > 1 (always k_rhs, fp64): h = H_x x + min_c (H_w w_c) + H_5
        B, S = 40, 3
        midx = rng.integers(0, 3, B).astype(np.int32)
        x0, om = rng.standard_normal((B, nx)), rng.standard_normal((B, S, nW))
        h = p.rhs(x0, om, midx, scenarios=S)
        for b in range(B):
            e = evos[midx[b]]
            hw = e["H_omega"] @ om[b].T if nW else np.zeros((N * d["nc"], S))
            ref = e["H_x"] @ x0[b] + hw.min(axis=1) + e["H_5"][:, 0]
            sc = np.abs(e["H_x"]) @ np.abs(x0[b]) + (np.abs(e["H_omega"]) @ np.abs(om[b]).T).max(axis=1) + np.abs(e["H_5"][:, 0])
            assert np.all(np.abs(h[b] - ref) <= 1e-12 * sc), (b, float((np.abs(h[b] - ref) / sc).max()))
    finally:
        p.close(); m.close()


# ------------------------------------------------------------------------------------------------------------------- K4
COST_PATHS = RHS_PATHS                        # k_gemm_mfma<false>, k_gemm (reserved bit 7), k_gemm_mfma<true> (MLD_F32)
# name -> (N, dims, n_models); GEMM sizes n = N nv, N nx, N ny, nx, N nw straddle the 16-wide MFMA tile and the 64-wide C tile
COST_SHAPES = {
    "below16": (5, dict(nx=3, nu=1, ndelta=1, nz=1, nomega=3, ny=3, nc=4), 7),        # n = N nx = N ny = N nw = 15
    "straddle64": (13, dict(nx=5, nu=3, ndelta=1, nz=1, nomega=5, ny=1, nc=4), 3),    # n = N nx = N nw = 65, N ny = 13
    "nx17": (4, dict(nx=17, nu=14, ndelta=1, nz=1, nomega=16, ny=4, nc=4), 1),        # n = N nw = 64, N nx = 68, N ny = 16
    "nw0": (9, dict(nx=7, nu=5, ndelta=1, nz=1, nomega=0, ny=2, nc=3), 3),            # n = N nx = 63, N ny = 18, no Qw
    "nx0": (6, dict(nx=0, nu=4, ndelta=1, nomega=4, ny=3, nc=4), 7),                  # no Gamma / Phi maps, no Qx: y terms only
}


def _check_cost(got, ref, fp32):
    for k in ("P", "q0", "Qx", "Qw"):
        r, g = ref[k], got[k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if r.size == 0:
            continue
        scale = float(np.abs(r).max())
        assert scale > 0, k
        err = float(np.abs(g - r).max())
        assert err <= (1e-5 if fp32 else 1e-11) * scale, (k, err / scale)
        if fp32 and k == "P":
            assert err > 1e-13 * scale                 # the fp32 GEMM really ran


def _cost_case(mats_list, d, N, horizons, path, seed):
    M = len(horizons) if horizons else len(mats_list)
    costs = [_paths.random_cost(seed + i, d, N) for i in range(M)]
    stacked = {k: (None if costs[0][k] is None else np.stack([c[k] for c in costs])) for k in costs[0]}
    m = gpu.GpuModel(horizons or mats_list, d, time_varying=bool(horizons))
    p = gpu.GpuProblem(m, N - 1, N, stacked, **dict(COST_PATHS)[path])
    try:
        got = p.cost_assemble()
    finally:
        p.close(); m.close()
    for i in range(M):
        evo = cn.condense_tv(horizons[i]) if horizons else cn.condense(mats_list[i], N)
        _check_cost({k: got[k][i] for k in got}, _paths.ref_cost(evo, **costs[i]), path == "mfma32")


@pytest.mark.parametrize("path", [p for p, _ in COST_PATHS])
@pytest.mark.parametrize("shape", list(COST_SHAPES))
def test_cost_assembly_paths(shape, path):
    """K4 through mld_cost_assemble with a different random non-symmetric quad_v, quad_x, quad_y and lin_v, lin_x, lin_y per
    model: k_symmetrize + the GEMM chain of set_cost_impl (per-model strides sA / sB / sC, the d_T scratch, beta = 1
    accumulation into P, q0, Qx, Qw) and k_pullback, on all three GEMM kernels, against ref_cost"""
    N, dims, M = COST_SHAPES[shape]
    seed = 2000 + 10 * list(COST_SHAPES).index(shape)
    mats, d = _models(M, seed, **dims)
    _cost_case(mats, d, N, None, path, seed)


@pytest.mark.parametrize("path", [p for p, _ in COST_PATHS])
def test_cost_assembly_time_varying_quadratic(path):
    """K4 on a time-varying handle (three horizons of independent step models, maps from k_tv_chain + k_tv_rows) with a
    quadratic cost on v, x and y"""
    N, dims = 8, dict(nx=4, nu=3, ndelta=1, nmu=1, nomega=2, ny=2, nc=4)
    horizons = [_paths.random_horizon(90 + i, N, **dims)[0] for i in range(3)]
    _cost_case(None, _paths.make_dims(**dims), N, horizons, path, 3000)
