"""A numpy restatement of the circulant-embedding sampler's contract (include/gsi_hip.h, gsi_gridcov_sampler_create;
DESIGN.md 4.6f): the torus covariance, its spectrum, neg_mass, the fields made from given noise -- and the case tables the
CPU and GPU tests share.  Arrays over the torus and the box are indexed [t0, t1(, t2)]; "vec" is Fortran order (t0 fastest),
the order of the C ABI."""
import collections
import itertools

import numpy as np

KINDS = {"gaussian": 0, "exponential": 1, "matern32": 2, "matern52": 3}
FIELD_BAR = 1e-12          # max |F - F_model| / max |F_model|: the FFTRF sampler's bar for the same line transform
COV_BAR = 1e-12            # max |F F' - C| / (sigma2 + nugget), and the spectrum's max |dlambda| / lambda_0

Case = collections.namedtuple("Case", "N M kind ell theta sigma2 nugget")


def case(N, M=None, kind="exponential", ell=1.0, theta=0.0, sigma2=1.0, nugget=0.0):
    N = tuple(int(v) for v in N)
    ell = (float(ell),) * len(N) if np.ndim(ell) == 0 else tuple(float(v) for v in ell)
    return Case(N, tuple(M) if M is not None else default_embed(N), kind, ell, float(theta), float(sigma2), float(nugget))


def case_id(c):
    return "x".join(map(str, c.N)) + "_on_" + "x".join(map(str, c.M)) + "_" + c.kind


def default_embed(N):
    """per axis the next power of two >= 2 N (the embedding of gsi_op_fft_gridcov)"""
    out = []
    for n in N:
        m = 2
        while m < 2 * n:
            m *= 2
        out.append(m)
    return tuple(out)


def kernel(kind, r):
    if kind == "gaussian":
        return np.exp(-0.5 * r * r)
    if kind == "exponential":
        return np.exp(-r)
    if kind == "matern32":
        a = np.sqrt(3.0) * r
        return (1.0 + a) * np.exp(-a)
    if kind == "matern52":
        a = np.sqrt(5.0) * r
        return (1.0 + a + a * a / 3.0) * np.exp(-a)
    raise ValueError(kind)


def cov_of_lags(c, lags):
    """sigma2 k(r) at the signed lags (one array per axis): u = the lag, in 2-D rotated by theta; r^2 = sum (u_a / ell_a)^2"""
    u = [np.asarray(s, dtype=np.float64) for s in lags]
    if len(u) == 2:
        cs, sn = np.cos(c.theta), np.sin(c.theta)
        u = [cs * u[0] + sn * u[1], -sn * u[0] + cs * u[1]]
    r2 = sum((ua / la) ** 2 for ua, la in zip(u, c.ell))
    return c.sigma2 * kernel(c.kind, np.sqrt(r2))


def torus_table(c):
    """c~(t) on the torus M: s_a = t_a if t_a <= M_a / 2, else t_a - M_a.  No nugget."""
    axes = []
    for m in c.M:
        t = np.arange(m)
        axes.append(np.where(t <= m // 2, t, t - m))
    return cov_of_lags(c, np.meshgrid(*axes, indexing="ij"))


def spectrum(c):
    """lambda_k = Re sum_t c~(t) exp(-2 pi i k.t / M) + nugget, shape M"""
    return np.fft.fftn(torus_table(c)).real + c.nugget


def neg_mass(c, lam):
    return float(-lam[lam < 0].sum() / (lam.size * (c.sigma2 + c.nugget)))


def fields_from_eps(lam, N, eps):
    """eps: Mtot x 2P, column c the noise of role c in vec order.  Returns n x 2P: columns 2 j, 2 j + 1 = Re, Im of
    w(t) = sum_k a_k (eps1_k + i eps2_k) exp(+2 pi i k.t / M) on the box, a_k = sqrt(max(lambda_k, 0) / Mtot)."""
    M = lam.shape
    mtot = lam.size
    a = np.sqrt(np.maximum(lam, 0.0) / mtot)
    box = tuple(slice(0, n) for n in N)
    out = np.empty((int(np.prod(N)), eps.shape[1]))
    for j in range(eps.shape[1] // 2):
        z = (eps[:, 2 * j] + 1j * eps[:, 2 * j + 1]).reshape(M, order="F")
        w = np.fft.ifftn(a * z) * mtot
        out[:, 2 * j] = w[box].real.reshape(-1, order="F")
        out[:, 2 * j + 1] = w[box].imag.reshape(-1, order="F")
    return out


def impulse_eps(mtot):
    """Noise (e_k, 0) for every k < Mtot: 2 Mtot fields F with F F' = the covariance of the sampler's fields."""
    eps = np.zeros((mtot, 2 * mtot), order="F")
    eps[np.arange(mtot), 2 * np.arange(mtot)] = 1.0
    return eps


def dense_cov(c):
    """The matrix of gsi_op_fft_gridcov: sigma2 k(r(i - j)) + nugget [i == j], points in vec order."""
    idx = np.array(list(itertools.product(*[range(n) for n in c.N[::-1]])))[:, ::-1]      # first axis fastest
    lags = [idx[:, None, a] - idx[None, :, a] for a in range(len(c.N))]
    return cov_of_lags(c, lags) + c.nugget * np.eye(len(idx))


# ---- the passes a case launches: (KIND, LR, SHORT) of csrc/gridcov_sample.hip ------------------------------------------
def pass_instantiations(c):
    """One (kind, LR, short) per axis: FIRST along axis 0, MIDDLE (3-D) along axis 1, LAST along the last axis; a line of M
    points runs the short kernel (one thread per line, LR = log2 M) below 16 points, else LR = log2 M mod 4."""
    out = []
    d = len(c.M)
    for a, m in enumerate(c.M):
        lg = int(m).bit_length() - 1
        assert 1 << lg == m and 2 <= m <= 8192
        kind = "FIRST" if a == 0 else ("LAST" if a == d - 1 else "MIDDLE")
        out.append((kind, lg if m < 16 else lg % 4, m < 16))
    return out


ALL_INSTANTIATIONS = {(k, lr, sh) for k in ("FIRST", "MIDDLE", "LAST")
                      for lr, sh in [(0, False), (1, False), (2, False), (3, False), (1, True), (2, True), (3, True)]}

# ---- the case tables -----------------------------------------------------------------------------------------------------
# exact: neg_mass = 0 in numpy, the impulse covariance equals the dense matrix to 1.2e-15
EXACT_CASES = [
    case((8, 4), (16, 8), "exponential", (2, 2)),
    case((8, 5), (16, 16), "exponential", (2.5, 1.2), theta=0.6, sigma2=1.7, nugget=0.01),
    case((9, 7), (32, 16), "matern32", (1.5, 0.8), theta=0.6),
    case((6, 5), (32, 16), "gaussian", (1.2, 0.9)),
    case((4, 3, 3), (8, 8, 8), "exponential", 0.8),
    case((4, 3, 2), (16, 8, 8), "matern52", (0.7, 0.6, 0.5)),
]
# the clamp's bound is attained on the diagonal: neg_mass = 0.0222802
BOUND_CASE = case((8, 8), (16, 16), "exponential", 10.0, sigma2=1.7)
BOUND_NEG_MASS = 0.0222802
# carried by the default embedding with neg_mass = 0 in numpy
DEFAULT_CASES = [
    case((24, 20), None, "exponential", 3.0),
    case((37, 29), None, "matern32", (6, 2), theta=0.6),
    case((32, 16), None, "exponential", (5, 2), theta=0.6),
    case((16, 12), None, "gaussian", 1.5),
    case((8, 6, 5), None, "exponential", 1.0),
    case((16, 12, 9), None, "matern52", 1.5),
]
DEFAULT_EMBEDS = {(24, 20): (64, 64), (37, 29): (128, 64)}
# not carried: neg_mass per torus
NOT_CARRIED = case((32, 32), None, "exponential", 40.0)
NOT_CARRIED_NEG_MASS = {64: 2.44e-2, 128: 7.56e-3, 256: 4.13e-4, 512: 0.0}


def _half(M):
    return tuple(max(1, m // 2) for m in M)


# the transform, every instantiation (positivity is irrelevant: neg_tol = 1, the expected fields use the device's spectrum)
TRANSFORM_CASES = (
    [case(_half(M), M, kind, ell) for M, kind, ell in [
        ((2, 4, 8), "exponential", 1.0), ((4, 8, 16), "gaussian", (1.0, 2.0, 1.5)), ((8, 16, 32), "matern32", 2.0),
        ((16, 32, 64), "exponential", (3.0, 2.0, 5.0)), ((32, 64, 128), "matern52", 4.0), ((64, 128, 2), "exponential", 6.0),
        ((128, 2, 4), "gaussian", 3.0)]]
    + [case((5, 3, 6), (16, 8, 32), "exponential", (2.0, 1.0, 3.0))]                      # N_a < M_a / 2 on every axis
    + [case(_half(M), M, "exponential", (7.0, 2.0), theta=0.4)
       for L, s in [(256, 2), (512, 4), (1024, 2), (2048, 4), (4096, 2), (8192, 4)] for M in [(L, s), (s, L)]]
)
GPU_CASES = EXACT_CASES + [BOUND_CASE] + DEFAULT_CASES + TRANSFORM_CASES
