"""Helpers for the kernel-path parity tests (tests/test_gpu_kernel_paths.py): random MLD models of chosen dimensions, the K4
cost pull-back written out directly from the condensed maps, and the fp32 error bound of K3.  CPU only; checked by
tests/test_kernel_path_refs.py."""
import numpy as np

MAT_SHAPES = dict(A=("nx", "nx"), B1=("nx", "nu"), B2=("nx", "ndelta"), B3=("nx", "nz"), B4=("nx", "nomega"), b5=("nx", 1),
                  C=("ny", "nx"), D1=("ny", "nu"), D2=("ny", "ndelta"), D3=("ny", "nz"), D4=("ny", "nomega"), d5=("ny", 1),
                  E=("nc", "nx"), F1=("nc", "nu"), F2=("nc", "ndelta"), F3=("nc", "nz"), F4=("nc", "nomega"), f5=("nc", 1),
                  G=("nc", "ny"), Psi=("nc", "nmu"))
EVO_NAMES = ("Phi_x", "Gamma_v", "Gamma_omega", "Gamma_5", "L_x", "L_v", "L_omega", "L_5", "H_x", "H_v", "H_omega", "H_5")
U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)


def make_dims(nx=0, nu=0, ndelta=0, nz=0, nmu=0, nomega=0, ny=0, nc=0):
    d = dict(nx=nx, nu=nu, ndelta=ndelta, nz=nz, nmu=nmu, nomega=nomega, ny=ny, nc=nc, nu_l=0, nmu_l=0)
    d["nv"] = nu + ndelta + nz + nmu
    return d


def spectral_radius(A):
    return float(np.abs(np.linalg.eigvals(A)).max()) if np.size(A) else 0.0


def random_mld(seed, rho=None, **dims):
    """one random MLD model with the given dimensions (any family may be empty).  Every matrix is standard normal scaled
    by 1/sqrt(its column count); A is rescaled to spectral radius `rho` (drawn from [0.9, 1.05] when not given), so that
    the late blocks of a long horizon stay O(1) and an error in them is not hidden under a global-max tolerance.
    Returns (mats, dims, rho)."""
    d = make_dims(**dims)
    rng = np.random.default_rng(seed)
    if rho is None:
        rho = float(rng.uniform(0.9, 1.05))
    mats = {}
    for name, (r, c) in MAT_SHAPES.items():
        rr, cc = d[r], (d[c] if isinstance(c, str) else c)
        mats[name] = rng.standard_normal((rr, cc)) / np.sqrt(max(1, cc))
    if d["nx"]:
        A = mats["A"]
        while spectral_radius(A) < 1e-3:            # (a nilpotent draw cannot be rescaled)
            A = rng.standard_normal(A.shape)
        mats["A"] = A * (rho / spectral_radius(A))
    return mats, d, rho


def random_horizon(seed, N, rho=None, **dims):
    """N independent random step models of the same dimensions (a time-varying horizon)"""
    out = [random_mld(seed * 1000 + k, rho=rho, **dims) for k in range(N)]
    return [m for m, _, _ in out], out[0][1]


def random_cost(seed, dims, N):
    """lin_v, lin_x, lin_y and NON-symmetric quad_v, quad_x, quad_y of one model (None where the family is empty)"""
    rng = np.random.default_rng(seed)
    n, lx, ly = N * dims["nv"], N * dims["nx"], N * dims["ny"]
    c = {}
    for k, ln in (("v", n), ("x", lx), ("y", ly)):
        c["lin_" + k] = rng.standard_normal(ln) if ln else None
        c["quad_" + k] = rng.standard_normal((ln, ln)) / np.sqrt(ln) if ln else None
    return c


def ref_cost(evo, lin_v=None, lin_x=None, lin_y=None, quad_v=None, quad_x=None, quad_y=None):
    """K4 restated from the condensed maps (x = Gamma_v v + Phi_x x0 + Gamma_w w + Gamma_5, same for y with L_*):
        P  = (Wv + Wv') + Gamma_v'(Wx + Wx')Gamma_v + L_v'(Wy + Wy')L_v
        q0 = lin_v + Gamma_v' lin_x + L_v' lin_y + Gamma_v'(Wx + Wx')Gamma_5 + L_v'(Wy + Wy')L_5
        Qx = Gamma_v'(Wx + Wx')Phi_x + L_v'(Wy + Wy')L_x ;  Qw = Gamma_v'(Wx + Wx')Gamma_w + L_v'(Wy + Wy')L_w"""
    n, nx, nW = evo["Gamma_v"].shape[1], evo["Phi_x"].shape[1], evo["Gamma_omega"].shape[1]
    P, q0, Qx, Qw = np.zeros((n, n)), np.zeros(n), np.zeros((n, nx)), np.zeros((n, nW))
    if lin_v is not None:
        q0 += np.asarray(lin_v, np.float64).reshape(n)
    if quad_v is not None:
        W = np.asarray(quad_v, np.float64).reshape(n, n)
        P += W + W.T
    for lin, quad, Mv, Mx, Mw, m5 in ((lin_x, quad_x, "Gamma_v", "Phi_x", "Gamma_omega", "Gamma_5"),
                                      (lin_y, quad_y, "L_v", "L_x", "L_omega", "L_5")):
        Mv, Mx, Mw, m5 = evo[Mv], evo[Mx], evo[Mw], evo[m5][:, 0]
        if Mv.shape[0] == 0:
            continue
        if lin is not None:
            q0 += Mv.T @ np.asarray(lin, np.float64).reshape(-1)
        if quad is not None:
            W = np.asarray(quad, np.float64).reshape(Mv.shape[0], Mv.shape[0])
            Ws = W + W.T
            P += Mv.T @ Ws @ Mv
            q0 += Mv.T @ (Ws @ m5)
            Qx += Mv.T @ Ws @ Mx
            Qw += Mv.T @ Ws @ Mw
    return dict(P=P, q0=q0, Qx=Qx, Qw=Qw)


def rhs_terms(evo, x0, omega):
    """h = H_x x0 + H_w w + H_5 and, per row, sum_j |H_ij z_j| over z = [x0; w; 1] (the scale every rounding error of the
    row is proportional to).  x0: (B, nx), omega: (B, N nw) -> both (B, m0)."""
    Hx, Hw, H5 = evo["H_x"], evo["H_omega"], evo["H_5"][:, 0]
    h = x0 @ Hx.T + omega @ Hw.T + H5
    s = np.abs(x0) @ np.abs(Hx).T + np.abs(omega) @ np.abs(Hw).T + np.abs(H5)
    return h, s


def fp32_dot_bound(K):
    """relative bound (times sum_j |H_ij z_j|) of an fp32 dot product of length K whose inputs are fp64 values rounded to
    fp32: each term carries two input roundings and one product rounding, the accumulation at most K - 1 more in any order,
    so |error| <= gamma_{K+2} sum|H_ij z_j| with gamma_k = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability of
    Numerical Algorithms, section 3.1)."""
    k = K + 2
    return k * U32 / (1.0 - k * U32)


def fuzz_mld(seed, **fix):
    """one seeded random MLD model that is NOT a tank cluster (tests/test_gpu_fuzz.py, tests/test_gpu_solver_paths.py): binary inputs and
    deltas, continuous auxiliaries, every row soft (Psi = -I).  `fix` overrides drawn dimensions (nx, nu, ndelta, nz, nomega, ny, nc); the
    draws themselves are unchanged, so without overrides a seed gives the model it always gave.  Returns (mats, dims, atoms, rng), the rng
    positioned for the instance draws."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    nx, nu, nd, nz = int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
    nw, ny, nc = int(rng.integers(0, 3)), int(rng.integers(1, 3)), int(rng.integers(3, 7))
    drawn = dict(nx=nx, nu=nu, ndelta=nd, nz=nz, nomega=nw, ny=ny, nc=nc)
    unknown = set(fix) - set(drawn)
    if unknown:
        raise TypeError("fuzz_mld: unknown dimension(s) %s" % sorted(unknown))
    drawn.update(fix)
    nx, nu, nd, nz, nw, ny, nc = (drawn[k] for k in ("nx", "nu", "ndelta", "nz", "nomega", "ny", "nc"))
    nmu = nc
    A = 0.8 * rng.standard_normal((nx, nx)) / max(1, nx) ** 0.5
    m = dict(A=A, B1=rng.standard_normal((nx, nu)), B2=rng.standard_normal((nx, nd)), B3=0.5 * rng.standard_normal((nx, nz)),
             B4=rng.standard_normal((nx, nw)), b5=0.1 * rng.standard_normal((nx, 1)),
             C=rng.standard_normal((ny, nx)), D1=rng.standard_normal((ny, nu)), D2=np.zeros((ny, nd)), D3=np.zeros((ny, nz)),
             D4=np.zeros((ny, nw)), d5=np.zeros((ny, 1)),
             E=rng.standard_normal((nc, nx)), F1=3.0 * rng.standard_normal((nc, nu)), F2=5.0 * rng.standard_normal((nc, nd)),
             F3=rng.standard_normal((nc, nz)), F4=0.3 * rng.standard_normal((nc, nw)), f5=1.0 + rng.random((nc, 1)),
             G=0.5 * rng.standard_normal((nc, ny)), Psi=-np.eye(nc))
    dims = dict(nx=nx, nu=nu, ndelta=nd, nz=nz, nmu=nmu, nomega=nw, ny=ny, nc=nc, nu_l=nu, nmu_l=0)
    atoms = {"q_mu": 5.0 + 10.0 * rng.random(nmu), "q_u": rng.standard_normal(nu)}
    if nd:
        atoms["q_delta"] = rng.standard_normal(nd)
    return m, dims, atoms, rng
