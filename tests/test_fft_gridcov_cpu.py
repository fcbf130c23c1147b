"""The FFT operator for covariance functions on a grid (gsi_op_fft_gridcov[_table]), without a GPU:

  * header, ctypes table and Julia shim carry the two new symbols (the static binding tests compare them argument by
    argument; here: that they are there at all);
  * the argument checks of api.cpp through the CPU reference build of the same C ABI: every bad argument is status 1
    (GSI_ERR_ARG) with a message that names it, and a valid call ends in the backend's "not supported by this backend"
    (the CPU reference backend does not have this operator) instead of a crash;
  * a numpy model of the plan construction -- the weighted cosine / sine factors D_a, S_a on the power-of-two embedding,
    (lambda' + nugget) / Mtot -- applied as the passes apply a plan, against the dense matrix of the header's formula.
"""
import ctypes as C

import numpy as np
import pytest

import cpuref
from test_binding_signatures_static import JULIA_FILES, header_prototypes, julia_ccalls

NEW = ("gsi_op_fft_gridcov", "gsi_op_fft_gridcov_table")


# ---------------------------------------------------------------- the three statements of the boundary
def test_header_ctypes_and_julia_shim_carry_the_new_symbols(gsi):
    protos = header_prototypes()
    bound = {c["name"] for c in julia_ccalls(JULIA_FILES[0])}
    for name in NEW:
        assert name in protos, name
        assert name in gsi._lib.SIGNATURES, name
        assert name in bound, f"{name} is not bound in the Julia shim"
    assert protos["gsi_op_fft_gridcov"] == ("i32", ["ptr", "ptr", "i32", "ptr", "i32", "ptr", "f64", "f64", "f64"])
    assert protos["gsi_op_fft_gridcov_table"] == ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "ptr", "f64"])
    assert "fft_gridcov_operator" in gsi.__all__ and callable(gsi.fft_gridcov_operator)


# ---------------------------------------------------------------- argument checks (api.cpp on the CPU reference backend)
@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    assert lib.gsi_backend_name().startswith(b"cpu-reference")
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()


def _err(gsi, fn):
    with pytest.raises(gsi.GsiError) as ei:
        fn()
    assert ei.value.code == 1, ei.value
    return str(ei.value)


@pytest.mark.parametrize("kwargs,word", [
    (dict(Ns=[8, 6], kind=4), "kind"),
    (dict(Ns=[8, 6], kind=-1), "kind"),
    (dict(Ns=[8, 6], ell=0.0), "ell"),
    (dict(Ns=[8, 6], ell=[2.0, -1.0]), "ell"),
    (dict(Ns=[8, 6], ell=[2.0, float("nan")]), "ell"),
    (dict(Ns=[8, 6], ell=float("inf")), "ell"),
    (dict(Ns=[8, 6], sigma2=0.0), "sigma2"),
    (dict(Ns=[8, 6], sigma2=float("inf")), "sigma2"),
    (dict(Ns=[8, 6], nugget=-1e-3), "nugget"),
    (dict(Ns=[8, 6], nugget=float("nan")), "nugget"),
    (dict(Ns=[8, 6], theta=float("nan")), "theta"),
    (dict(Ns=[12], theta=0.3), "theta"),
    (dict(Ns=[4, 5, 6], theta=0.3), "theta"),
    (dict(Ns=[4, 5, 6, 7]), "grid dimensions"),
    (dict(Ns=[4, 0]), "grid dimensions"),
    (dict(Ns=[1, 1]), "two grid points"),
    (dict(Ns=[5000]), "4096 grid points per axis"),
    (dict(Ns=[8, 1 << 40]), "4096 grid points per axis"),
])
def test_bad_arguments_are_refused_by_name(gsi, cx, kwargs, word):
    msg = _err(gsi, lambda: gsi.fft_gridcov_operator(cx, **kwargs))
    assert word in msg, msg
    assert "not supported by this backend" not in msg


def test_bad_tables_are_refused_by_name(gsi, cx):
    t = np.exp(-np.hypot(*np.meshgrid(np.arange(8.0), np.arange(6.0), indexing="ij")) / 3.0)
    bad = t.copy(); bad[3, 2] = np.nan
    assert "table entries must be finite" in _err(gsi, lambda: gsi.fft_gridcov_operator(cx, [8, 6], table=bad))
    assert "table_mirror entries must be finite" in _err(gsi, lambda: gsi.fft_gridcov_operator(cx, [8, 6], table=t, table_mirror=bad))
    assert "nugget" in _err(gsi, lambda: gsi.fft_gridcov_operator(cx, [8, 6], table=t, nugget=-1.0))
    m = t.copy(); m[3, 0] *= 1.0 + 1e-9                       # the same lag (t1 == 0) with another value
    assert "t1 == 0" in _err(gsi, lambda: gsi.fft_gridcov_operator(cx, [8, 6], table=t, table_mirror=m))
    m = t.copy(); m[0, 4] += 1e-6                             # c(0, -t1) != c(0, t1): not centrally symmetric
    assert "t0 == 0" in _err(gsi, lambda: gsi.fft_gridcov_operator(cx, [8, 6], table=t, table_mirror=m))
    t3 = np.ones((3, 4, 5))
    assert "table_mirror" in _err(gsi, lambda: gsi.fft_gridcov_operator(cx, [3, 4, 5], table=t3, table_mirror=t3))
    # NULL pointers where an array is read (below the Python layer)
    h = C.c_void_p()
    N = (C.c_int64 * 2)(8, 6)
    assert cx.lib.gsi_op_fft_gridcov_table(cx.h, C.byref(h), 2, N, None, None, 0.0) == 1
    assert b"table is NULL" in cx.lib.gsi_last_error()
    assert cx.lib.gsi_op_fft_gridcov(cx.h, C.byref(h), 2, N, 1, None, 0.0, 1.0, 0.0) == 1
    assert b"ell is NULL" in cx.lib.gsi_last_error()
    assert cx.lib.gsi_op_fft_gridcov(cx.h, C.byref(h), 2, None, 1, None, 0.0, 1.0, 0.0) == 1
    with pytest.raises(ValueError):
        gsi.fft_gridcov_operator(cx, [8, 6], table=t[:, :5])
    with pytest.raises(ValueError):
        gsi.fft_gridcov_operator(cx, [8, 6], ell=[1.0, 2.0, 3.0])


def test_valid_calls_reach_the_backend_which_does_not_have_the_operator(gsi, cx):
    before = cx.device_bytes()
    for kw in (dict(Ns=[8, 6], kind="matern52", ell=[2.0, 3.0], theta=0.6, sigma2=1.7, nugget=0.01),
               dict(Ns=[9, 6, 11], kind=0, ell=2.0), dict(Ns=[50], kind="exponential", ell=7.0),
               dict(Ns=[8, 6], table=np.ones((8, 6)), table_mirror=np.ones((8, 6)))):
        assert "not supported by this backend" in _err(gsi, lambda: gsi.fft_gridcov_operator(cx, **kw))
    assert cx.device_bytes() == before


# ---------------------------------------------------------------- numpy model of the plan
def _k(kind, r):
    """The four kernels of csrc/pointcov.hpp (the header's definition of kind 0..3)."""
    if kind == 0:
        return np.exp(-0.5 * r * r)
    if kind == 1:
        return np.exp(-r)
    a = np.sqrt(3.0 if kind == 2 else 5.0) * r
    return (1.0 + a) * np.exp(-a) if kind == 2 else (1.0 + a + a * a / 3.0) * np.exp(-a)


def cov_of_lags(Ns, kind, ell, theta, sigma2, t):
    """sigma2 k(r) at integer lags t (list of arrays, one per axis): the header's formula."""
    u = [np.asarray(x, dtype=float) for x in t]
    if theta != 0.0:
        assert len(Ns) == 2
        u = [np.cos(theta) * u[0] + np.sin(theta) * u[1], -np.sin(theta) * u[0] + np.cos(theta) * u[1]]
    r2 = sum((ua / la) ** 2 for ua, la in zip(u, ell))
    return sigma2 * _k(kind, np.sqrt(r2))


def dense_matrix(Ns, kind, ell, theta, sigma2, nugget):
    """A(i, j) = sigma2 k(r) + nugget [i == j], point index column-major."""
    idx = np.unravel_index(np.arange(int(np.prod(Ns))), Ns, order="F")
    t = [ia[:, None] - ia[None, :] for ia in idx]
    return cov_of_lags(Ns, kind, ell, theta, sigma2, t) + nugget * np.eye(len(idx[0]))


def _embed(N):
    m = 1
    while m < 2 * N:
        m <<= 1
    return 1 if N == 1 else m


def _factor(N, M, sine):
    """D_a[k', t] = w_t cos(2 pi t k' / M), S_a likewise with sin; w_0 = 1, w_t = 2; exact argument reduction."""
    t, k = np.arange(N), np.arange(M)
    arg = 2.0 * np.pi * ((k[:, None] * t[None, :]) % M) / M
    w = np.where(t > 0, 2.0, 1.0)[None, :]
    return w * (np.sin(arg) if sine else np.cos(arg))


def _apply_factors(c, Ms, sine):
    for a, M in enumerate(Ms):
        c = np.moveaxis(np.tensordot(_factor(c.shape[a], M, sine), c, axes=(1, a)), 0, a)
    return c


def plan_spectrum(Ns, cp, cm, nugget):
    """What the plan stores: (lambda' + nugget) / Mtot, lambda' = (x D_a) c or (D_0 x D_1) c_ee - (S_0 x S_1) c_oo."""
    Ms = [_embed(N) for N in Ns]
    if cm is None:
        lam = _apply_factors(cp, Ms, False)
    else:
        lam = _apply_factors(0.5 * (cp + cm), Ms, False) - _apply_factors(0.5 * (cp - cm), Ms, True)
    return (lam + nugget) / float(np.prod(Ms)), Ms


def plan_apply(lam_over_mtot, Ns, Ms, X):
    """The passes: zero-pad to the embedding, forward FFT, multiply, UNNORMALISED inverse (the 1 / Mtot is in the plan), restrict."""
    Y = np.empty_like(X)
    box = tuple(slice(0, N) for N in Ns)
    for j in range(X.shape[1]):
        w = np.zeros(Ms)
        w[box] = X[:, j].reshape(Ns, order="F")
        y = np.fft.ifftn(np.fft.fftn(w) * lam_over_mtot) * float(np.prod(Ms))
        Y[:, j] = y.real[box].reshape(-1, order="F")
    return Y


def lag_tables(Ns, kind, ell, theta, sigma2):
    g = np.meshgrid(*[np.arange(N) for N in Ns], indexing="ij")
    cp = cov_of_lags(Ns, kind, ell, theta, sigma2, g)
    cm = cov_of_lags(Ns, kind, ell, theta, sigma2, [g[0], -g[1]]) if theta != 0.0 else None
    return cp, cm


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("Ns,ell,theta", [((50,), (7.0,), 0.0), ((37, 29), (6.0, 2.5), 0.0), ((37, 29), (6.0, 2.5), 0.6),
                                          ((9, 6, 11), (3.0, 2.0, 4.0), 0.0), ((5, 2, 3), (3.0, 2.0, 4.0), 0.0)])
def test_plan_model_against_the_dense_matrix(kind, Ns, ell, theta):
    """37 x 29 with theta = 0.6 embeds to 128 x 64.  Bound: the FFT's own rounding on these sizes is a few 1e-15 of max|Y|;
    1e-12 is the bar the GPU tests hold the passes to."""
    sigma2, nugget = 1.7, 0.01
    A = dense_matrix(Ns, kind, ell, theta, sigma2, nugget)
    cp, cm = lag_tables(Ns, kind, ell, theta, sigma2)
    lam, Ms = plan_spectrum(Ns, cp, cm, nugget)
    assert np.isrealobj(lam)
    X = np.random.default_rng(int(np.prod(Ns)) + kind).standard_normal((A.shape[0], 5))
    Y = plan_apply(lam, Ns, Ms, X)
    Yref = A @ X
    assert np.abs(Y - Yref).max() < 1e-12 * np.abs(Yref).max()


def test_the_nugget_is_the_identity_on_the_box_and_the_diagonal_is_not_normalised():
    Ns, ell = (12, 9), (3.0, 2.0)
    cp, _ = lag_tables(Ns, 1, ell, 0.0, 2.5)
    lam0, Ms = plan_spectrum(Ns, cp, None, 0.0)
    lam1, _ = plan_spectrum(Ns, cp, None, 0.3)
    E = np.eye(int(np.prod(Ns)))
    A0, A1 = plan_apply(lam0, Ns, Ms, E), plan_apply(lam1, Ns, Ms, E)
    assert np.abs(A1 - A0 - 0.3 * E).max() < 1e-13
    assert np.abs(np.diag(A0) - 2.5).max() < 1e-13


def test_a_mirrored_table_is_needed_for_a_rotated_kernel():
    """With the even-axes construction alone a rotated kernel comes out wrong by O(1): the odd-odd term is not a refinement."""
    Ns, ell, theta = (16, 12), (6.0, 2.0), 0.6
    A = dense_matrix(Ns, 0, ell, theta, 1.0, 0.0)
    cp, cm = lag_tables(Ns, 0, ell, theta, 1.0)
    X = np.random.default_rng(1).standard_normal((A.shape[0], 3))
    lam, Ms = plan_spectrum(Ns, cp, None, 0.0)
    assert np.abs(plan_apply(lam, Ns, Ms, X) - A @ X).max() > 1e-2 * np.abs(A @ X).max()
    lam, Ms = plan_spectrum(Ns, cp, cm, 0.0)
    assert np.abs(plan_apply(lam, Ns, Ms, X) - A @ X).max() < 1e-12 * np.abs(A @ X).max()
