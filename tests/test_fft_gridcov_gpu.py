"""The FFT operator for covariance functions on a grid (gsi_op_fft_gridcov[_table]) on the MI355X.

Tolerances are the project's bars for the same quantities: 1e-12 of max|Y| for a product through the passes
(test_fft_powerlaw_operator), 1e-9 / 1e-6 for randsvd against the oracle (test_implicit_gridcov_randsvd).  numpy's FFT alone
stays between 1.4e-16 and 2.0e-15 on the shapes, kinds and angles below."""
import numpy as np
import pytest

from oracle import oracle as orc
from helpers import gaussian_cov, rel_sv_err
from test_fft_gridcov_cpu import dense_matrix, lag_tables

pytestmark = pytest.mark.gpu

KINDS = ["gaussian", "exponential", "matern32", "matern52"]


@pytest.fixture(scope="module")
def ctx(gsi):
    c = gsi.default_context()
    yield c


def _close(Y, Yref, what=""):
    err, scale = np.abs(Y - Yref).max(), np.abs(Yref).max()
    print(f"{what} max|Y - Yref| / max|Yref| = {err / scale:.2e}")
    assert err < 1e-12 * scale, (what, err / scale)


# 1. the stored matrix of the same grid covariance
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("ny,nx,l", [(40, 33, 5), (40, 33, 160), (64, 50, 200), (130, 7, 48)])
def test_against_the_stored_grid_covariance(gsi, ctx, ny, nx, l, kind):
    """N = (ny, nx) is gridcov_operator(nx, ny) in the same point order; odd and even column counts (two real columns ride
    in one complex transform)."""
    ell = 4.0
    n = nx * ny
    X = np.random.default_rng(n + l).standard_normal((n, l))
    dense = gsi.gridcov_operator(ctx, nx, ny, ell, kind)
    op = gsi.fft_gridcov_operator(ctx, [ny, nx], kind=kind, ell=ell)
    assert op.shape == (n, n)
    Yref = dense.matmul(X)
    _close(op.matmul(X), Yref, "A X")
    _close(op.rmatmul_t(X), dense.rmatmul_t(X), "A' X")
    op.close(); dense.close()


# 2. the dense matrix of the header's formula
SHAPES = [((50,), (7.0,)), ((37, 29), (6.0, 2.5)), ((40, 64), (3.0, 9.0)), ((9, 6, 11), (3.0, 2.0, 4.0)),
          ((3, 1100), (2.0, 40.0)), ((2, 3), (1.5, 2.0)), ((5, 2, 3), (3.0, 2.0, 4.0))]
CASES = [(Ns, ell, 0.0) for Ns, ell in SHAPES] + [((37, 29), (6.0, 2.5), 0.6), ((40, 64), (3.0, 9.0), 0.6)]
# a singleton axis is squeezed out of the passes but keeps its ell and its place in the rotation
CASES += [((1, 50), (2.0, 7.0), 0.0), ((1, 50), (2.0, 7.0), 0.6), ((6, 1, 9), (2.0, 5.0, 3.0), 0.0)]


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("Ns,ell,theta", CASES)
def test_against_the_dense_matrix_of_the_formula(gsi, ctx, Ns, ell, theta, kind):
    sigma2, nugget = 1.7, 0.01
    n = int(np.prod(Ns))
    A = dense_matrix(Ns, kind, ell, theta, sigma2, nugget)
    op = gsi.fft_gridcov_operator(ctx, Ns, kind=KINDS[kind], ell=ell, theta=theta, sigma2=sigma2, nugget=nugget)
    X = np.random.default_rng(n + kind).standard_normal((n, 7))
    Yref = A @ X
    _close(op.matmul(X), Yref, "A X")
    _close(op.rmatmul_t(X), Yref, "A' X")
    # symmetry and the diagonal on unit vectors: columns of A itself
    cols = sorted({0, 1, n // 2, n - 1} | set(np.random.default_rng(3).integers(0, n, 6).tolist()))
    E = np.zeros((n, len(cols)))
    E[cols, np.arange(len(cols))] = 1.0
    Ac = op.matmul(E)
    assert np.abs(Ac[cols, :] - Ac[cols, :].T).max() < 1e-12 * (sigma2 + nugget)
    assert np.abs(Ac[cols, np.arange(len(cols))] - (sigma2 + nugget)).max() < 1e-12
    _close(Ac, A[:, cols], "columns of A")
    op.close()


# 3. tables
def test_table_of_a_nested_kernel_against_the_implicit_operator(gsi, ctx):
    ny, nx = 64, 50
    n = nx * ny
    dx, dy = np.meshgrid(np.arange(nx, dtype=float), np.arange(ny, dtype=float), indexing="ij")
    d = np.hypot(dx, dy)
    table = 0.7 * np.exp(-0.5 * (d / 5.0) ** 2) + 0.3 * np.exp(-d / 20.0)          # table[dx, dy]: nx x ny, C order
    impl = gsi.gridcov_implicit_operator(ctx, nx, ny, 1.0, table=table)
    op = gsi.fft_gridcov_operator(ctx, [ny, nx], table=table.T)                  # the same bytes: t[dx * ny + dy]
    X = np.random.default_rng(9).standard_normal((n, 33))
    _close(op.matmul(X), impl.matmul(X), "table A X")
    _close(op.rmatmul_t(X), impl.rmatmul_t(X), "table A' X")
    opn = gsi.fft_gridcov_operator(ctx, [ny, nx], table=table.T, nugget=0.25)
    _close(opn.matmul(X), impl.matmul(X) + 0.25 * X, "table + nugget")
    op.close(); opn.close(); impl.close()


@pytest.mark.parametrize("Ns,ell", [((37, 29), (6.0, 2.5)), ((40, 64), (3.0, 9.0))])
def test_mirrored_table_is_the_theta_constructor(gsi, ctx, Ns, ell):
    theta, sigma2, nugget = 0.6, 1.7, 0.01
    n = int(np.prod(Ns))
    cp, cm = lag_tables(Ns, 2, ell, theta, sigma2)
    a = gsi.fft_gridcov_operator(ctx, Ns, kind="matern32", ell=ell, theta=theta, sigma2=sigma2, nugget=nugget)
    b = gsi.fft_gridcov_operator(ctx, Ns, table=cp, table_mirror=cm, nugget=nugget)
    X = np.random.default_rng(4).standard_normal((n, 6))
    _close(b.matmul(X), a.matmul(X), "mirror vs theta")
    _close(b.matmul(X), dense_matrix(Ns, 2, ell, theta, sigma2, nugget) @ X, "mirror vs dense")
    a.close(); b.close()


def test_inconsistent_mirror_is_refused(gsi, ctx):
    Ns = (12, 10)
    cp, cm = lag_tables(Ns, 1, (3.0, 2.0), 0.6, 1.0)
    bad = cm.copy(); bad[0, 4] *= 1.0 + 1e-6
    before = ctx.device_bytes()
    with pytest.raises(gsi.GsiError, match="t0 == 0"):
        gsi.fft_gridcov_operator(ctx, Ns, table=cp, table_mirror=bad)
    bad = cm.copy(); bad[5, 0] += 1e-6
    with pytest.raises(gsi.GsiError, match="t1 == 0"):
        gsi.fft_gridcov_operator(ctx, Ns, table=cp, table_mirror=bad)
    assert ctx.device_bytes() == before


# 4. the whole 10^6-point matrix against an independent implementation
def test_the_headline_matrix_against_the_implicit_operator(gsi, ctx):
    """1000 x 1000, exponential, ell = 100, the X of test_implicit_gridcov_at_the_headline_size: every one of the 10^6 rows
    against the implicit operator's product (entries regenerated inside the MFMA contraction: no code shared with the FFT
    passes), and that test's 52 host-computed rows with its bar."""
    g, ell, l = 1000, 100.0, 16
    n = g * g
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.standard_normal((n, l)))
    impl = gsi.gridcov_implicit_operator(ctx, g, g, ell, kind=1)
    Yi = impl.matmul(X)
    impl.close()
    op = gsi.fft_gridcov_operator(ctx, [g, g], kind="exponential", ell=ell)
    Y = op.matmul(X)
    Yt = op.rmatmul_t(X)
    op.close()
    scale = np.abs(Yi).max()
    err = np.abs(Y - Yi).max()
    print(f"max|Y_fft - Y_implicit| / max|Y| = {err / scale:.2e} over {n} rows")
    assert err < 1e-12 * scale
    assert np.abs(Yt - Yi).max() < 1e-12 * scale
    px, py = np.divmod(np.arange(n), g)                        # point = x * ny + y (tests/helpers.py:grid_points)
    rows = np.concatenate([[0, 1, g - 1, g, n // 2, n - g, n - 1, 4295, 65535, 65536, 262143, 262144],
                           rng.integers(0, n, size=40)])
    worst = worst_impl = 0.0
    for i in rows:
        a = np.exp(-np.sqrt((px - px[i]) ** 2.0 + (py - py[i]) ** 2.0) / ell)
        ref = a @ X
        worst = max(worst, np.abs(Y[i] - ref).max() / scale)
        worst_impl = max(worst_impl, np.abs(Yi[i] - ref).max() / scale)
        assert np.abs(Y[i] - ref).max() < 1e-12 * scale, i
        assert np.abs(Yt[i] - ref).max() < 1e-12 * scale, i
    print(f"host rows: worst {worst:.2e} (the implicit operator's own product on these rows: {worst_impl:.2e})")


# 5. randsvd
def test_randsvd_through_the_fft_operator(gsi, ctx):
    nx, ny, ell, K, p, q = 48, 40, 4.0, 20, 12, 2
    n = nx * ny
    Om = np.random.default_rng(3).standard_normal((n, K + p))
    op = gsi.fft_gridcov_operator(ctx, [ny, nx], kind="gaussian", ell=ell)
    Z, S = gsi.randsvd(op, K, p, q, Omega=Om, return_S=True)
    A = gaussian_cov(nx, ny, ell)
    Zr, Sr, _ = orc.randsvd_full(A, K, p, q, Om)
    assert rel_sv_err(S, Sr, K) < 1e-9
    assert orc.xis_error_up_to_sign(Z, Zr, K) < 1e-6
    assert np.all(Z[:, K:] == 0)
    op.close()


# 6. limits and memory
def test_limits_are_refused_before_anything_is_allocated(gsi, ctx):
    before = ctx.device_bytes()
    with pytest.raises(gsi.GsiError, match=r"fewer than 2\^31"):
        gsi.fft_gridcov_operator(ctx, [1024, 512, 512], ell=10.0)
    assert ctx.device_bytes() == before
    with pytest.raises(gsi.GsiError, match="4096 grid points per axis"):
        gsi.fft_gridcov_operator(ctx, [5000], ell=10.0)
    with pytest.raises(gsi.GsiError, match="theta"):
        gsi.fft_gridcov_operator(ctx, [10, 10, 10], ell=3.0, theta=0.5)
    assert ctx.device_bytes() == before


def test_creating_and_closing_leaves_no_device_memory_behind(gsi, ctx):
    cases = (dict(Ns=[300, 200], kind="matern52", ell=[20.0, 8.0], theta=0.6, nugget=0.1), dict(Ns=[30, 20, 10], ell=4.0))

    def cycle(check_above=None):
        for kw in cases:
            op = gsi.fft_gridcov_operator(ctx, **kw)
            op.matmul(np.random.default_rng(0).standard_normal((op.shape[0], 3)))
            if check_above is not None:
                assert ctx.device_bytes() > check_above
            op.close()
        ctx.release_cache()
        return ctx.device_bytes()

    # The context keeps the contraction kernel's split-K workspace at the largest size it has seen, and release_cache returns
    # it only when it is above 64 MiB: that is the context's memory, not an operator's.  So: drop what earlier work left,
    # let one cycle bring the workspace to the (small) size these plans need, and the next two must leave exactly that.
    ctx.release_cache()
    before = cycle()
    assert cycle(check_above=before) == before
    assert cycle(check_above=before) == before
