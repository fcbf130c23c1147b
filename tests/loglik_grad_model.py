"""Dense models of the likelihood gradient, in numpy longdouble where it matters:

  * `dk_entries`: the entries of d(sigma2 k(r) + nugget I) / d param of `gsi_op_fft_gridcov_deriv`, restating
    csrc/pointcov.hpp's `dprofile` / `dkernel` (ONE function, `dprofile`, carries the kernel family);
  * `cov_entries`: the covariance itself in longdouble (the kernels of tests/test_fft_gridcov_cpu.py), for finite differences;
  * `loglik` and `loglik_grad`: the dense REML / ML log-likelihood through `slogdet` and its analytic gradient;
  * `same_probe_terms`: the S_k and t_{k,i} that `log_likelihood_grad` estimates, from dense inverses with the same probes;
  * `richardson`: central differences with two Richardson steps (error O(h^6)).
"""
import numpy as np

LD = np.longdouble
KINDS = ["gaussian", "exponential", "matern32", "matern52"]
PARAMS = ["log_sigma2", "log_ell", "log_ell0", "log_ell1", "log_ell2", "theta", "nugget"]


def _ld(x):
    return np.asarray(x, dtype=LD)


def kernel(kind, r):
    r = _ld(r)
    if kind == 0:
        return np.exp(-r * r / 2)
    if kind == 1:
        return np.exp(-r)
    a = np.sqrt(LD(3 if kind == 2 else 5)) * r
    return (1 + a) * np.exp(-a) if kind == 2 else (1 + a + a * a / 3) * np.exp(-a)


def dprofile(kind, r):
    """g(r) = -k'(r) / r; the exponential kernel's g(0) is defined as 0."""
    r = _ld(r)
    if kind == 0:
        return np.exp(-r * r / 2)
    if kind == 1:
        safe = np.where(r > 0, r, LD(1))
        return np.where(r > 0, np.exp(-r) / safe, LD(0))
    if kind == 2:
        return 3 * np.exp(-np.sqrt(LD(3)) * r)
    a = np.sqrt(LD(5)) * r
    return LD(5) / 3 * (1 + a) * np.exp(-a)


def lags(Ns):
    """The integer lags i - j per axis, n x n each, point index column-major."""
    idx = np.unravel_index(np.arange(int(np.prod(Ns))), Ns, order="F")
    return [_ld(ia[:, None] - ia[None, :]) for ia in idx]


def scaled(Ns, ell, theta, t):
    """(u_a / ell_a) per axis (three entries), rotated in 2-D."""
    ell = [LD(v) for v in ell]
    u = list(t)
    if len(Ns) == 2:
        th = LD(theta)
        u = [np.cos(th) * t[0] + np.sin(th) * t[1], -np.sin(th) * t[0] + np.cos(th) * t[1]]
    else:
        assert theta == 0.0
    out = [ua / la for ua, la in zip(u, ell)]
    while len(out) < 3:
        out.append(np.zeros_like(out[0]))
    return out


def cov_entries(Ns, kind, ell, theta, sigma2, nugget, t=None):
    t = lags(Ns) if t is None else t
    u = scaled(Ns, ell, theta, t)
    r = np.sqrt(u[0] ** 2 + u[1] ** 2 + u[2] ** 2)
    same = np.ones_like(r, dtype=bool)
    for ta in t:
        same &= (ta == 0)
    return LD(sigma2) * kernel(kind, r) + LD(nugget) * same


def dk_entries(Ns, kind, ell, theta, sigma2, param, t=None):
    """d (sigma2 k(r) + nugget [i == j]) / d param, longdouble, n x n (or the shape of the lags `t`)."""
    t = lags(Ns) if t is None else t
    u = scaled(Ns, ell, theta, t)
    q = [ua ** 2 for ua in u]
    r2 = q[0] + q[1] + q[2]
    r = np.sqrt(r2)
    if param == "nugget":
        same = np.ones_like(r, dtype=bool)
        for ta in t:
            same &= (ta == 0)
        return _ld(same)
    if param == "log_sigma2":
        return LD(sigma2) * kernel(kind, r)
    g = LD(sigma2) * dprofile(kind, r)
    if param == "log_ell":
        return g * r2
    if param in ("log_ell0", "log_ell1", "log_ell2"):
        return g * q[int(param[-1])]
    assert param == "theta" and len(Ns) == 2
    rot = LD(ell[1]) / LD(ell[0]) - LD(ell[0]) / LD(ell[1])
    return -(g * u[0] * u[1]) * rot


def richardson(f, x, h):
    """f'(x) from central differences at h, h / 2 and h / 4, extrapolated twice: error O(h^6)."""
    d = [(f(x + h / k) - f(x - h / k)) / (2 * h / k) for k in (1, 2, 4)]
    e1, e2 = (4 * d[1] - d[0]) / 3, (4 * d[2] - d[1]) / 3
    return (16 * e2 - e1) / 15


def fd_entries(Ns, kind, ell, theta, sigma2, param, h=LD(1) / 64, t=None):
    """The same derivative by `richardson` on `cov_entries` (not for "nugget", which is linear)."""
    t = lags(Ns) if t is None else t
    ell = [LD(v) for v in ell]

    def f(x):
        e, th, s2 = list(ell), LD(theta), LD(sigma2)
        if param == "log_sigma2":
            s2 = np.exp(x)
        elif param == "log_ell":
            e = [v * np.exp(x) for v in ell]
        elif param == "theta":
            th = x
        else:
            a = int(param[-1])
            e[a] = np.exp(x)
        return cov_entries(Ns, kind, e, th, s2, 0, t=t)

    x0 = {"log_sigma2": np.log(LD(sigma2)), "log_ell": LD(0), "theta": LD(theta)}.get(param)
    if x0 is None:
        x0 = np.log(ell[int(param[-1])])
    return richardson(f, x0, LD(h))


# ---- the dense likelihood ------------------------------------------------------------------------------------------------
def loglik(M, y, G, restricted=True):
    """The value `log_likelihood` estimates, from the dense M (float64 `slogdet`)."""
    M = np.asarray(M, dtype=np.float64)
    m, p = y.size, G.shape[1]
    Mi_y = np.linalg.solve(M, y)
    ld = np.linalg.slogdet(M)[1]
    if p:
        Mi_G = np.linalg.solve(M, G)
        GMG = G.T @ Mi_G
        beta = np.linalg.solve(GMG, G.T @ Mi_y)
        r = y - G @ beta
        q = r @ (Mi_y - Mi_G @ beta)
        if restricted:
            return -0.5 * (q + ld + np.linalg.slogdet(GMG)[1] + (m - p) * np.log(2 * np.pi))
        return -0.5 * (q + ld + m * np.log(2 * np.pi))
    return -0.5 * (y @ Mi_y + ld + m * np.log(2 * np.pi))


def loglik_grad(M, dMs, y, G, restricted=True):
    """The analytic gradient: -1/2 [tr(M^-1 dM) - tr((G'M^-1 G)^-1 G'M^-1 dM M^-1 G) - xi' dM xi], longdouble inverses."""
    Ml = _ld(M)
    Mi = _ld(np.linalg.inv(np.asarray(M, dtype=np.float64)))
    Mi = Mi @ (2 * np.eye(M.shape[0], dtype=LD) - Ml @ Mi)         # one Newton step in longdouble
    Mi = Mi @ (2 * np.eye(M.shape[0], dtype=LD) - Ml @ Mi)
    yl, Gl = _ld(y), _ld(G)
    p = G.shape[1]
    if p:
        MiG = Mi @ Gl
        GMG = Gl.T @ MiG
        GMGi = _ld(np.linalg.inv(np.asarray(GMG, dtype=np.float64)))
        GMGi = GMGi @ (2 * np.eye(p, dtype=LD) - GMG @ GMGi)
        beta = GMGi @ (Gl.T @ (Mi @ yl))
        xi = Mi @ (yl - Gl @ beta)
    else:
        xi = Mi @ yl
    out = []
    for dM in dMs:
        dl = _ld(dM)
        v = np.sum(Mi * dl.T) - xi @ dl @ xi
        if restricted and p:
            v -= np.trace(GMGi @ (MiG.T @ dl @ MiG))
        out.append(-v / 2)
    return np.asarray(out, dtype=np.float64)


def same_probe_terms(M, dMs, y, G, Z, P=None):
    """S_k = X0' dM X0 and t_{k,i} = x_i' dM w_i with X = M^-1 [y, G, Z], W = P^-1 Z, from dense float64 solves."""
    M = np.asarray(M, dtype=np.float64)
    X = np.linalg.solve(M, np.column_stack([y, G, Z]))
    g = 1 + G.shape[1]
    W = Z if P is None else np.linalg.solve(P, Z)
    S = [X[:, :g].T @ np.asarray(dM, dtype=np.float64) @ X[:, :g] for dM in dMs]
    T = np.array([np.einsum("ij,ij->j", X[:, g:], np.asarray(dM, dtype=np.float64) @ W) for dM in dMs])
    return S, T, X


def grad_from_terms(S, T, X, y, G, restricted=True):
    """What `log_likelihood_grad` forms from S_k, t_k and the solved columns X = M^-1 [y, G, ...]."""
    p = G.shape[1]
    if p:
        GMG = G.T @ X[:, 1:1 + p]
        beta = np.linalg.solve(GMG, G.T @ X[:, 0])
    else:
        GMG, beta = np.zeros((0, 0)), np.zeros(0)
    c = np.concatenate([[1.0], -beta])
    out = []
    for Sk, tk in zip(S, T):
        mid = np.trace(np.linalg.solve(GMG, Sk[1:, 1:])) if (restricted and p) else 0.0
        out.append(-0.5 * (np.mean(tk) - mid - c @ Sk @ c))
    return np.array(out)
