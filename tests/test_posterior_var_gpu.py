"""The posterior variance on the device: the row pass of posterior_var.hip through
gsi_basis_quadform -- every edge to the bounds of posterior_cases.py, exact integers, reproducibility and row independence,
64-bit offsets, path reporting -- and the feature on top of it: the variance against the dense saddle-point formula in extended
precision, the factor, the observed-point property, the realisations and the errors."""
import ctypes as C

import numpy as np
import pytest

import posterior_cases as pc

pytestmark = pytest.mark.gpu
DEVICE, HOST = 1, 3


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()


@pytest.fixture(autouse=True)
def _device_path(monkeypatch):
    monkeypatch.delenv("GSI_POST_HOST", raising=False)


# ---- 1, 2: every edge, to the derived bounds and exactly ----------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("K", pc.K_LIST)
def test_row_sums_within_the_bounds(gsi, ctx, K, precision):
    worst = 0.0
    for n in pc.N_LIST:
        Z, _ = pc.kernel_inputs(n, K, False)
        basis, Zs = pc.make_basis(gsi, ctx, Z, precision)
        worst = max(worst, pc.check_kernel_case(basis, Zs, False, (n, K, precision), DEVICE))
        pc.close_basis(basis)
    print(f"K={K} fp{precision}: largest error / bound {worst:.3g}")


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("K", pc.K_LIST)
def test_row_sums_exact_on_integers(gsi, ctx, K, precision):
    for n in pc.N_LIST:
        Z, _ = pc.kernel_inputs(n, K, True)
        basis, Zs = pc.make_basis(gsi, ctx, Z, precision)
        assert np.array_equal(Zs, Z)
        pc.check_kernel_case(basis, Zs, True, (n, K, precision), DEVICE)
        pc.close_basis(basis)


def test_two_column_chunks_of_a_triangular_w(gsi, ctx):
    """K = 2 chunks + 5 with a triangular W: the second and third chunk start below the diagonal and skip whole tiles."""
    K, n = 2 * pc.COL_CHUNK + 5, pc.ROW_TILE + 3
    Z, u = pc.kernel_inputs(n, K, True)
    basis, Zs = pc.make_basis(gsi, ctx, Z, 64)
    Wu = np.triu(np.random.default_rng(8).integers(-3, 4, (K, K)).astype(np.float64))
    Wp = np.asfortranarray(Wu + np.tril(np.full((K, K), np.nan), -1))
    a, q, t = basis.quadform(Wp, u, upper=True)
    pc.close_basis(basis)
    ref = pc.kernel_reference(Zs, Wu, u)
    assert np.array_equal(a, ref["a"].astype(np.float64))
    assert np.array_equal(q, ref["q"].astype(np.float64)) and np.array_equal(t, ref["t"].astype(np.float64))


# ---- 3: reproducibility and row independence ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_same_bits_twice_and_rows_do_not_depend_on_n(gsi, ctx, precision):
    n, K = 3 * pc.ROW_TILE + 9, 37
    Z, u = pc.kernel_inputs(n, K, False)
    W = np.asfortranarray(np.random.default_rng(3).standard_normal((K, K + 3)))
    basis, _ = pc.make_basis(gsi, ctx, Z, precision)
    first = basis.quadform(W, u)
    second = basis.quadform(W, u)
    pc.close_basis(basis)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)
    for m in (pc.ROW_TILE - 1, pc.ROW_TILE, pc.ROW_TILE + 1, 2 * pc.ROW_TILE, 17):
        part, _ = pc.make_basis(gsi, ctx, Z[:m], precision)       # a basis is column-major: built from the first m rows
        got = part.quadform(W, u)
        pc.close_basis(part)
        for x, y in zip(first, got):
            assert np.array_equal(x[:m], y), m


# ---- 4: 64-bit offsets ------------------------------------------------------------------------------------------------------
def test_offsets_beyond_4_gib(gsi, ctx):
    """n = 2^22 + 7, K = 130: 4.36 GB in fp64.  Z is zero except integer rows in a 64-row window around the 4 GiB byte offset,
    which falls into column 127, and the last 5 rows."""
    n, K = 2 ** 22 + 7, 130
    col, off = divmod(2 ** 29, n)
    assert col == 127
    rows = np.concatenate([np.arange(off - 32, off + 32), np.arange(n - 5, n)])
    rng = np.random.default_rng(17)
    Zr = rng.integers(-3, 4, (rows.size, K)).astype(np.float64)
    W = np.asfortranarray(rng.integers(-3, 4, (K, K)).astype(np.float64))
    u = rng.integers(-3, 4, K).astype(np.float64)
    try:
        Zm = gsi.DeviceMatrix(ctx, n, K)
    except gsi.GsiError as e:
        if e.code == 6:
            pytest.skip("the device has less than the 12 GB this case needs free")
        raise
    Z = np.zeros((n, K), order="F")
    Z[rows] = Zr
    gsi._lib.check(ctx.lib.gsi_mat_upload(ctx.h, Zm.h, gsi._lib.dptr(Z), n), ctx.lib)
    del Z
    basis = gsi.DeviceBasis(Zm, K)
    a, q, t, info = basis.quadform(W, u, return_info=True)
    basis.close()
    Zm.close()
    assert info == [0, DEVICE]
    P = Zr @ W
    assert np.array_equal(a[rows], (P * P).sum(axis=1))
    assert np.array_equal(q[rows], (Zr * Zr).sum(axis=1)) and np.array_equal(t[rows], Zr @ u)
    a[rows] = q[rows] = t[rows] = 0.0
    assert np.count_nonzero(a) == 0 and np.count_nonzero(q) == 0 and np.count_nonzero(t) == 0


# ---- 5: path reporting ------------------------------------------------------------------------------------------------------
def test_host_path_when_asked_and_the_two_agree(gsi, ctx, monkeypatch):
    n, K = 200, 65
    Z, u = pc.kernel_inputs(n, K, False)
    basis, Zs = pc.make_basis(gsi, ctx, Z, 64)
    W = np.asfortranarray(np.random.default_rng(4).standard_normal((K, K)))
    ref = pc.kernel_reference(Zs, W, u)
    dev = basis.quadform(W, u, return_info=True)
    monkeypatch.setenv("GSI_POST_HOST", "1")
    host = basis.quadform(W, u, return_info=True)
    monkeypatch.delenv("GSI_POST_HOST")
    pc.close_basis(basis)
    assert dev[3] == [0, DEVICE] and host[3] == [0, HOST]
    for got in (dev, host):
        assert pc.worst_ratio(got[0], ref["a"], ref["ba"]) <= 1.0
        assert pc.worst_ratio(got[1], ref["q"], ref["bq"]) <= 1.0
        assert pc.worst_ratio(got[2], ref["t"], ref["bt"]) <= 1.0


# ---- 6 - 9: the feature ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", pc.FEATURE_CASES)
def test_variance_against_the_dense_formula(gsi, ctx, name, precision, with_prior):
    ratio = pc.check_variance(gsi, ctx, name, precision, with_prior, DEVICE)
    print(f"{name} fp{precision} prior={with_prior}: max |v - v_ref| / max |v_ref| = {ratio:.3g}")
    assert ratio <= pc.VARIANCE_BAR


@pytest.mark.parametrize("name", pc.FEATURE_CASES)
def test_factor_and_scalars(gsi, ctx, name):
    r = pc.check_factor(gsi, ctx, name, DEVICE)
    print(f"{name}: |W'NW - I| {r[0]:.3g}, u {r[1]:.3g}, gamma {r[2]:.3g}")


@pytest.mark.parametrize("precision", [64, 32])
def test_observed_points_are_no_worse_than_their_measurement(gsi, ctx, precision):
    print(f"fp{precision}: max v / R_jj = {pc.check_observed_points(gsi, ctx, precision, DEVICE):.4f}")


@pytest.mark.parametrize("on_device", [True, False])
def test_realizations_and_the_covariance_identity(gsi, ctx, on_device):
    r = pc.check_realizations(gsi, ctx, on_device)
    print(f"realisations {r[0]:.3g}, covariance identity {r[1]:.3g}")


def test_variance_on_the_host_path_agrees(gsi, ctx, monkeypatch):
    monkeypatch.setenv("GSI_POST_HOST", "1")
    ratio = pc.check_variance(gsi, ctx, "n500_points", 64, False, HOST)
    assert ratio <= pc.VARIANCE_BAR


# ---- 10: errors; none of them launches the kernel on bad input -------------------------------------------------------------
def _matrix(gsi, ctx, rd, hx=None, nobs=6, K=3):
    rng = np.random.default_rng(4)
    E = np.asfortranarray(rng.standard_normal((nobs, K)))
    hx = rng.standard_normal(nobs) if hx is None else hx
    dp = gsi._lib.dptr
    h = C.c_void_p()
    assert ctx.lib.gsi_pcgamat_create(ctx.h, C.byref(h), dp(E), nobs, K, dp(hx), dp(rd), 1) == 0
    return h


def _variance_status(gsi, ctx, basis, h):
    X, v = np.ones(basis.n), np.full(basis.n, -7.0)
    info = (C.c_int64 * 2)()
    dp = gsi._lib.dptr
    st = ctx.lib.gsi_pcga_posterior_variance(ctx.h, basis.h, h, dp(X), None, dp(v), info)
    return st, list(info), v, ctx.lib.gsi_last_error()


def test_errors(gsi, ctx):
    basis, _ = pc.make_basis(gsi, ctx, np.random.default_rng(1).standard_normal((70, 3)), 64)
    rd = np.full(6, 0.5)
    rd[2] = 0.0
    h = _matrix(gsi, ctx, rd)
    st, info, v, msg = _variance_status(gsi, ctx, basis, h)
    assert st == 7 and info[0] == 3 and b"3" in msg and np.all(v == -7.0)          # a zero diagonal entry of R: its column
    ctx.lib.gsi_pcgamat_destroy(h)
    h = _matrix(gsi, ctx, np.full(6, 0.5), hx=np.zeros(6))
    st, info, v, msg = _variance_status(gsi, ctx, basis, h)
    assert st == 3 and np.all(v == -7.0)                                            # HX = 0
    ctx.lib.gsi_pcgamat_destroy(h)
    other = gsi.Context(ctx.device)
    try:
        h = _matrix(gsi, other, np.full(6, 0.5))
        st, info, v, msg = _variance_status(gsi, ctx, basis, h)
        assert st == 1 and b"another context" in msg and np.all(v == -7.0)
        other.lib.gsi_pcgamat_destroy(h)
    finally:
        other.close()
    dp = gsi._lib.dptr
    a = np.empty(70)
    W = np.asfortranarray(np.eye(3))
    assert ctx.lib.gsi_basis_quadform(ctx.h, basis.h, None, 3, 3, 0, None, dp(a), None, None, None) == 1
    assert ctx.lib.gsi_basis_quadform(ctx.h, basis.h, dp(W), 3, 3, 0, None, None, None, None, None) == 1
    assert ctx.lib.gsi_basis_quadform(ctx.h, basis.h, dp(W), 3, 3, 0, dp(a), dp(a), None, None, None) == 1   # u without t_out
    assert ctx.lib.gsi_pcga_posterior_variance(ctx.h, basis.h, None, dp(a), None, dp(a), None) == 1
    pc.close_basis(basis)


# ---- 11: the variance and the row sums are one row pass ----------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_variance_and_quadform_share_the_row_pass(gsi, ctx, precision):
    """gsi_pcga_posterior_variance and gsi_basis_quadform with the same triangular W and u (those of gsi_pcgamat_posterior)
    run the same row pass: the a, q and t behind the variance are the bits gsi_basis_quadform returns.  The variance is
    a + (t - X)^2 / gamma, plus prior - q with a prior; X = t makes the second term vanish and leaves a, prior = q makes the
    prior term vanish (the difference of two nearby doubles is exact, so another q would show), and X = 0 is compared with
    the same formula evaluated in the same order on the row sums."""
    import scipy.sparse as sp
    n, K, nobs = 257, 33, 40
    Z, _ = pc.kernel_inputs(n, K, False)
    rng = np.random.default_rng(33)
    A = gsi.PCGALowRankMatrix([rng.standard_normal(nobs) for _ in range(K)], rng.standard_normal(nobs),
                              sp.diags(rng.uniform(0.5, 1.5, nobs), format="csc"), ctx=ctx)
    basis, _ = pc.make_basis(gsi, ctx, Z, precision)
    dp = gsi._lib.dptr

    def variance(X, prior):
        v = np.empty(n)
        info = (C.c_int64 * 2)()
        st = ctx.lib.gsi_pcga_posterior_variance(ctx.h, basis.h, A.h, dp(X), dp(prior) if prior is not None else None, dp(v), info)
        assert st == 0 and list(info) == [0, DEVICE], (st, list(info))
        return v

    try:
        W, u, gamma, info = A.posterior_factor(return_info=True)
        assert info == [0, DEVICE]
        a, q, t, info = basis.quadform(W, u, upper=True, return_info=True)
        assert info == [0, DEVICE]
        assert np.array_equal(variance(t, None), a)
        assert np.array_equal(variance(t, q), a)
        assert np.array_equal(variance(np.zeros(n), None), a + t * t / gamma)
        shifted = q + 1.0
        assert np.array_equal(variance(np.zeros(n), shifted), (shifted - q) + (a + t * t / gamma))
    finally:
        A.close()
        pc.close_basis(basis)
