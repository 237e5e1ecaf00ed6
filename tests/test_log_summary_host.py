"""CPU tests of the campaign KPIs (pyhybridcontrol_amd/simlog.py: KpiTable, summary_np; the rule of pyhybridcontrol_amd/csrc/log_summary.inc): the numpy
restatement against a second, vectorised statement on random records with skipped rows, the edge cases of the accumulate rule, the shape and refusal checks
of KpiTable, the ABI, and the stand-alone host check of the rule's C functions under the address and undefined-behaviour sanitizers.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

from pyhybridcontrol_amd import _lib, simlog
from pyhybridcontrol_amd.simlog import KpiTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = dict(nx=3, nu=3, ndelta=1, nz=1, nmu=6, nomega=4, ny=1, nc=12)
NV = 11


def _random_log(rng, K, B, skipped):
    """records as GpuProblem.sim_log() returns them; skipped (K, B) bool: NaN in v, y, x_k1 and cons_vio, as k_sim_step marks a skipped instance"""
    log = dict(x=rng.normal(size=(K, B, 3)), v=rng.normal(size=(K, B, NV)), y=rng.normal(size=(K, B, 1)), omega=rng.normal(size=(K, B, 4)),
               x_k1=rng.normal(size=(K, B, 3)), cons_vio=rng.normal(scale=1e-6, size=(K, B)), nodes=rng.integers(0, 50, (K, B)).astype(np.int32))
    for name in ("v", "y", "x_k1", "cons_vio"):
        log[name][skipped] = np.nan
    return log


def _vectorised(log, arr, midx, price, source, vio_tol):
    """the summary in numpy's own order: einsum per table, nan-aware reductions over the stepped records"""
    K, B = log["cons_vio"].shape
    f = 0.0
    for key, name in zip(simlog.KPI_TABLES, ("x", "v", "y", "omega", "x_k1")):
        if arr[key] is not None:
            f = f + np.einsum("bqi,kbi->kbq", arr[key][midx], np.nan_to_num(log[name]))
    for q in np.flatnonzero(arr["price_chan"] >= 0):
        f[:, :, q] *= price[:, :, arr["price_chan"][q]]
    stepped = ~np.isnan(log["x_k1"][:, :, 0])
    on = stepped[:, :, None]
    thr = np.inf if arr["thresh"] is None else arr["thresh"][midx][None]
    out = dict(sum=np.where(on, f, 0.0).sum(axis=0), min=np.where(on, f, np.inf).min(axis=0), max=np.where(on, f, -np.inf).max(axis=0),
               n_above=(on & (f > thr)).sum(axis=0), n_stepped=stepped.sum(axis=0), nodes_total=log["nodes"].astype(np.int64).sum(axis=0))
    out["min_step"] = np.where(out["n_stepped"][:, None] > 0, np.where(on, f, np.inf).argmin(axis=0), -1)
    out["max_step"] = np.where(out["n_stepped"][:, None] > 0, np.where(on, f, -np.inf).argmax(axis=0), -1)
    vio = np.where(stepped, log["cons_vio"], -np.inf)
    out["vio_max"], out["n_vio"] = vio.max(axis=0), (stepped & (log["cons_vio"] > vio_tol)).sum(axis=0)
    out["vio_step"] = np.where(np.isfinite(out["vio_max"]), vio.argmax(axis=0), -1)
    out["n_source"] = np.stack([(source == s).sum(axis=0) for s in range(3)], axis=1)
    changes = np.zeros(f.shape[1:], np.int64)
    for b in range(B):
        rows = f[stepped[:, b], b]
        changes[b] = (rows[1:] != rows[:-1]).sum(axis=0) if rows.shape[0] > 1 else 0
    out["n_changes"] = changes
    return out


def _table(rng, M=2):
    t = KpiTable(M, DIMS)
    t.add("x_only", w_x=rng.normal(size=3))
    t.add("v_only", w_v=rng.normal(size=(M, NV)), thresh=0.1)
    t.add("y_only", w_y=np.ones(1), thresh=np.array([0.0, 0.5]))
    t.add("omega_only", w_omega=rng.normal(size=4))
    t.add("xk1_only", w_xk1=rng.normal(size=(M, 3)))
    t.add("all_five", w_x=rng.normal(size=3), w_v=rng.normal(size=NV), w_y=rng.normal(size=1), w_omega=rng.normal(size=4), w_xk1=rng.normal(size=3), thresh=0.0)
    t.add("priced", w_v=rng.normal(size=NV), price_chan=1)
    t.add("switch", w_v=np.eye(NV)[0])
    return t


def test_summary_np_equals_a_vectorised_statement():
    rng = np.random.default_rng(9400)
    K, B, M = 9, 13, 2
    skipped = rng.uniform(size=(K, B)) < 0.3
    skipped[:, 0], skipped[:, 1] = True, False                                  # an all-skipped instance and one that is never skipped
    log = _random_log(rng, K, B, skipped)
    log["v"][:, :, 0] = np.where(skipped, np.nan, rng.integers(0, 2, (K, B)))   # a switching channel
    midx = (np.arange(B) % M).astype(np.int32)
    price, source = rng.uniform(0.5, 2.0, (K, B, 2)), rng.integers(-1, 3, (K, B)).astype(np.int32)
    t = _table(rng, M)
    got = simlog.summary_np(log, t, midx, price=price, source=source, vio_tol=5e-7, first=4)
    ref = _vectorised(log, t.arrays(), midx, price, source, 5e-7)
    assert got["names"] == t.names and got["sum"].shape == (B, len(t)) and got["min_step"].dtype == np.int32 and got["nodes_total"].dtype == np.int64
    # sums of at most 5 tables x 11 terms and 9 records in two orders: (terms + records) * 2^-52 of the sum of the absolute terms, below 1e-12 here
    for name in ("sum", "min", "max", "vio_max"):
        assert np.allclose(got[name], ref[name], rtol=1e-12, atol=1e-12), name
    for name in ("n_above", "n_changes", "n_stepped", "n_vio", "nodes_total", "n_source"):
        assert np.array_equal(got[name], ref[name]), name
    for name in ("min_step", "max_step", "vio_step"):
        assert np.array_equal(got[name], np.where(ref[name] >= 0, ref[name] + 4, -1)), name          # absolute record indices
    # the all-skipped instance: the empty values
    assert got["n_stepped"][0] == 0 and np.all(got["sum"][0] == 0) and np.all(got["min"][0] == np.inf) and np.all(got["max"][0] == -np.inf)
    assert np.all(got["min_step"][0] == -1) and np.all(got["max_step"][0] == -1) and got["vio_max"][0] == -np.inf and got["vio_step"][0] == -1
    assert got["n_stepped"][1] == K and got["n_changes"][:, t.names.index("switch")].max() > 0
    # without a source array: -1
    assert np.all(simlog.summary_np(log, t, midx, price=price)["n_source"] == -1)
    with pytest.raises(ValueError, match="needs price"):
        simlog.summary_np(log, t, midx)


def test_ties_nan_and_the_empty_range():
    t = KpiTable(1, DIMS).add("u0", w_v=np.eye(NV)[0], thresh=0.5)
    vals = np.array([1.0, -2.0, 5.0, np.nan, -2.0, 5.0, 5.0])                   # ties at 1 / 4 (min) and 2 / 5 / 6 (max), a skipped record at 3
    K = vals.size
    log = dict(x=np.zeros((K, 1, 3)), v=np.zeros((K, 1, NV)), y=np.zeros((K, 1, 1)), omega=np.zeros((K, 1, 4)), x_k1=np.zeros((K, 1, 3)),
               cons_vio=np.array([0.0, 2.0, 2.0, np.nan, 1.0, 2.0, -1.0]).reshape(K, 1), nodes=np.full((K, 1), 2 ** 30, np.int32))
    log["v"][:, 0, 0] = vals
    log["x_k1"][3] = np.nan
    out = simlog.summary_np(log, t, None, first=10)
    assert out["sum"][0, 0] == 12.0 and out["n_stepped"][0] == 6
    assert (out["min"][0, 0], out["min_step"][0, 0], out["max"][0, 0], out["max_step"][0, 0]) == (-2.0, 11, 5.0, 12)      # the first attaining record
    assert out["n_above"][0, 0] == 4 and out["n_changes"][0, 0] == 4            # 1 -> -2 -> 5 -> (skipped) -> -2 -> 5 -> 5
    assert (out["vio_max"][0], out["vio_step"][0], out["n_vio"][0]) == (2.0, 11, 4) and out["nodes_total"][0] == 7 * 2 ** 30
    # a NaN value in a stepped record never wins, and reaches the sum
    log["x_k1"][3] = 0.0
    out = simlog.summary_np(log, t, None, first=10)
    assert np.isnan(out["sum"][0, 0]) and out["min_step"][0, 0] == 11 and out["max_step"][0, 0] == 12 and out["n_changes"][0, 0] == 5
    # count == 0
    empty = {k: a[:0] for k, a in log.items()}
    out = simlog.summary_np(empty, t, None)
    assert out["sum"].shape == (1, 1) and out["sum"][0, 0] == 0.0 and out["min"][0, 0] == np.inf and out["max"][0, 0] == -np.inf
    assert out["min_step"][0, 0] == -1 and out["n_stepped"][0] == 0 and out["vio_max"][0] == -np.inf and out["nodes_total"][0] == 0


def test_kpi_table_shapes_and_refusals():
    t = KpiTable(2, DIMS)
    t.add("a", w_v=np.arange(NV, dtype=float)).add("b", w_x=np.ones((2, 3)), thresh=1.0, price_chan=0)
    arr = t.arrays()
    assert arr["w_v"].shape == (2, 2, NV) and arr["w_x"].shape == (2, 2, 3) and arr["w_y"] is None and arr["w_omega"] is None and arr["w_xk1"] is None
    assert np.array_equal(arr["w_v"][1, 0], np.arange(NV)) and not arr["w_v"][:, 1].any() and not arr["w_x"][:, 0].any()
    assert np.array_equal(arr["price_chan"], [-1, 0]) and arr["price_chan"].dtype == np.int32
    assert np.array_equal(arr["thresh"], [[np.inf, 1.0], [np.inf, 1.0]]) and len(t) == 2 and t.names == ["a", "b"]
    assert KpiTable(1, DIMS).add("a", w_x=np.ones(3)).arrays()["thresh"] is None
    with pytest.raises(ValueError, match="added already"):
        t.add("a", w_x=np.ones(3))
    with pytest.raises(ValueError, match="no table given"):
        t.add("c")
    with pytest.raises(ValueError, match="w_v has shape"):
        t.add("c", w_v=np.ones(NV + 1))
    with pytest.raises(ValueError, match="w_x has shape"):
        t.add("c", w_x=np.ones((3, 3)))
    with pytest.raises(ValueError, match="non-finite"):
        t.add("c", w_y=np.array([np.inf]))
    with pytest.raises(ValueError, match="thresh"):
        t.add("c", w_y=np.ones(1), thresh=np.nan)
    with pytest.raises(ValueError, match="price_chan"):
        t.add("c", w_y=np.ones(1), price_chan=-1)
    with pytest.raises(ValueError, match="none of that variable"):
        KpiTable(1, dict(DIMS, ny=0)).add("c", w_y=np.ones(1))
    with pytest.raises(ValueError, match="holds no KPI"):
        KpiTable(1, DIMS).arrays()
    assert len(t) == 2                                                          # a refused add leaves the table as it was
    full = KpiTable(1, DIMS)
    for q in range(simlog.KPI_MAX):
        full.add("k%d" % q, w_x=np.ones(3))
    with pytest.raises(ValueError, match="at most 64"):
        full.add("one more", w_x=np.ones(3))


def test_microgrid_columns():
    t = KpiTable.microgrid(DIMS, n_models=2, price_chan=0)
    assert t.names == ["p_imp", "p_exp", "cost", "mu_over", "mu_under", "u_0", "u_1", "u_2"]
    arr = t.arrays()
    z = 4
    v = np.arange(1.0, NV + 1)
    assert arr["w_v"][0, 0] @ v == v[z] and arr["w_v"][0, 1] @ v == -v[z] and arr["w_y"][0, 1, 0] == 1.0 and not arr["w_y"][0, [0, 2, 3]].any()
    assert arr["w_v"][1, 3] @ v == v[5] + v[7] + v[9] and arr["w_v"][1, 4] @ v == v[6] + v[8] + v[10] and arr["w_v"][0, 6] @ v == v[1]
    assert np.array_equal(arr["price_chan"], [-1, -1, 0, -1, -1, -1, -1, -1]) and np.all(arr["thresh"][:, 3:5] == 0.0)
    assert "cost" not in KpiTable.microgrid(DIMS).names
    with pytest.raises(ValueError, match="grid tie"):
        KpiTable.microgrid(dict(DIMS, nz=0))


def test_abi_declares_and_binds_the_entry_point():
    assert "mld_sim_log_summary" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "mldgpu.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint mld_sim_log_summary\(mld_problem_t \*, int first, int count, int n_kpi,", header)
    assert re.search(r"#define MLD_KPI_MAX 64\b", header) and simlog.KPI_MAX == 64
    with open(os.path.join(ROOT, "pyhybridcontrol_amd", "_lib.py")) as fh:
        assert "lib.mld_sim_log_summary.argtypes" in fh.read()


def test_host_check_is_clean_under_the_sanitizers(tmp_path):
    """scripts/log_summary_host_check.cpp, its own executable: the C functions k_log_summary calls, under ASan and UBSan"""
    exe = str(tmp_path / "log_summary_host_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pyhybridcontrol_amd", "csrc"),
           os.path.join(ROOT, "scripts", "log_summary_host_check.cpp"), "-o", exe]
    # the runtimes linked into the program where the compiler can (the executable then stands alone), as shared libraries otherwise
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert ran.returncode == 0 and "as stated" in ran.stdout, ran.stdout
