"""The auxiliaries of synthetic.make_agent(..., tie=True) in closed form (tests/test_sim_resolve_host.py checks it against the C oracle,
tests/test_gpu_sim_resolve.py uses it against the device): what MldModel._compute_aux (models/mld_model.py:701-766) finds for (x, u, omega) once the total
slack is minimal.  With y = D1 u + omega_load the grid-tie rows of make_agent are the big-M statement of delta = [y >= 0], z = delta y, and the tank rows
x_i - mu_top_i <= T_max_i, -x_i - mu_bot_i <= -T_min_i leave mu_top = max(0, x - T_max), mu_bot = max(0, T_min - x) as the least slack.  CPU only."""
import numpy as np


def _g(mats, k, r, c):
    return np.zeros((r, c)) if mats.get(k) is None or np.size(mats[k]) == 0 else np.asarray(mats[k], float).reshape(r, c)


def closed_form(mats, dims, x, u, omega):
    """x (B, nx), u (B, nu), omega (B, nomega) -> dict(y (B,), delta (B, 1), z (B, 1), mu (B, 2 nx) [top_0, bot_0, top_1, ...], v (B, 2 + 2 nx))"""
    n_h = dims["nx"]
    x, u, omega = (np.asarray(a, float).reshape(-1, w) for a, w in ((x, n_h), (u, dims["nu"]), (omega, dims["nomega"])))
    y = u @ _g(mats, "D1", 1, dims["nu"])[0] + omega[:, n_h]
    f5 = _g(mats, "f5", dims["nc"], 1)[:, 0]
    t_max, t_min = f5[0:2 * n_h:2], -f5[1:2 * n_h:2]
    mu = np.zeros((x.shape[0], 2 * n_h))
    mu[:, 0::2], mu[:, 1::2] = np.maximum(0.0, x - t_max), np.maximum(0.0, t_min - x)
    delta, z = (y >= 0).astype(float)[:, None], np.maximum(y, 0.0)[:, None]
    return dict(y=y, delta=delta, z=z, mu=mu, v=np.hstack([delta, z, mu]))


def residual(mats, d, x, u, om, dl, z, mu):
    """the reference's own feasibility statement (mld_model.py:735-744) for one triple and one point: E x + F1 u + F2 delta + F3 z + F4 omega + G y + Psi mu - f5"""
    nx, ny, nc = d["nx"], d["ny"], d["nc"]
    y = _g(mats, "C", ny, nx) @ x + _g(mats, "D1", ny, d["nu"]) @ u + _g(mats, "D2", ny, d["ndelta"]) @ dl + _g(mats, "D3", ny, d["nz"]) @ z + \
        _g(mats, "D4", ny, d["nomega"]) @ om + _g(mats, "d5", ny, 1)[:, 0]
    return (_g(mats, "E", nc, nx) @ x + _g(mats, "F1", nc, d["nu"]) @ u + _g(mats, "F2", nc, d["ndelta"]) @ dl + _g(mats, "F3", nc, d["nz"]) @ z +
            _g(mats, "F4", nc, d["nomega"]) @ om + _g(mats, "G", nc, ny) @ y + _g(mats, "Psi", nc, d["nmu"]) @ mu - _g(mats, "f5", nc, 1)[:, 0])


def draw_triples(ag, B, rng):
    """(x, u, omega) of one agent: tank temperatures on and beside the integers between the soft bounds' reach (some below T_min, some above T_max = 65),
    u Bernoulli(0.4), omega step 0 of a forecast row with the load channel moved by N(0, 800) -- a realised load that is not the forecast's"""
    d = ag["dims"]
    x = rng.integers(50, 66, size=(B, d["nx"])).astype(float) + rng.choice([0.0, -3.0, 0.5], size=(B, d["nx"]))
    u = (rng.uniform(size=(B, d["nu"])) < 0.4).astype(float)
    om = ag["omega"][rng.integers(0, ag["omega"].shape[0], B), :d["nomega"]].copy()
    om[:, d["nx"]] += rng.normal(0.0, 800.0, B)
    return x, u, om


def hard_variant(mats, dims):
    """the model with its soft rows made hard: Psi zeroed and nmu = 0, so E x <= T_max must hold as it is -- a tank above T_max has no feasible auxiliaries"""
    m = {k: v for k, v in mats.items() if k != "Psi"}
    return m, dict(dims, nmu=0, nmu_l=0)
