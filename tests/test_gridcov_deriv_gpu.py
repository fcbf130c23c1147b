"""The derivative grid operators (`gsi_op_fft_gridcov_deriv`, csrc/fft_gridcov_plan.hip:fft_lag_table_deriv_kernel) and the
shared points plan (`gsi_op_fft_at_like`) on the MI355X.

Products on identity columns -- the columns of the matrix itself -- against the dense longdouble model of
tests/loglik_grad_model.py, which tests/test_loglik_grad_model.py checks against differences of the kernels.  The bar is the
project's for a product through the FFT passes: 1e-12 max|Y_ref| (test_fft_gridcov_gpu._close), and through `fft_operator_at`
and `linear_data_operator` those tests' own bars, which are the same figure.  A derivative that is identically zero (theta
with equal lengths) is held to 1e-12 of the largest entry of the covariance."""
import itertools

import numpy as np
import pytest

import fftrf_interp_model as im
import fwd_cov_cases as fc
import interp_adjoint_model as am
import loglik_grad_cases as lc
import loglik_grad_model as lm
import solve_cases as sc

pytestmark = pytest.mark.gpu

SIGMA2 = 1.7
# (Ns, ell, theta): a line, 2-D, rotated 2-D with unequal lengths (the mirror table), 3-D, an axis of one point (squeezed
# out of the passes, kept in the formula), short and long lengths
CASES = [((5,), (2.0,), 0.0), ((7, 5), (3.0, 1.5), 0.0), ((7, 5), (3.0, 1.5), 0.4), ((3, 4, 5), (3.0, 2.0, 4.0), 0.0),
         ((1, 6), (2.0, 3.0), 0.0), ((1, 6), (2.0, 3.0), 0.4), ((4, 1, 3), (2.0, 5.0, 3.0), 0.0),
         ((7, 5), (0.05, 0.05), 0.0), ((7, 5), (50.0, 50.0), 0.0)]
RATIOS = {}


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()
    lc.write_errors("derivative_operators_ratio_to_bar", RATIOS)


def _record(key, value):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(value))


def applicable(param, ndims):
    if param == "theta":
        return ndims == 2
    if param in ("log_ell0", "log_ell1", "log_ell2"):
        return int(param[-1]) < ndims
    return True


def _columns(op):
    n = op.shape[0]
    return op.matmul(np.eye(n))


@pytest.mark.parametrize("kind", range(4))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_every_param_against_the_dense_model(gsi, ctx, case, kind):
    Ns, ell, theta = CASES[case]
    n = int(np.prod(Ns))
    cov_scale = SIGMA2
    per_axis = np.zeros((n, n))
    for param in lm.PARAMS:
        if not applicable(param, len(Ns)):
            continue
        ref = lm.dk_entries(Ns, kind, ell, theta, SIGMA2, param).astype(np.float64)
        op = gsi.fft_gridcov_derivative(ctx, Ns, param, kind=lm.KINDS[kind], ell=ell, theta=theta, sigma2=SIGMA2)
        try:
            assert op.shape == (n, n) and op.Ns == tuple(Ns)
            Y = _columns(op)
        finally:
            op.close()
        assert np.isfinite(Y).all(), (param, "the r = 0 entry and every other must be finite")
        scale = max(float(np.abs(ref).max()), 0.0)
        bar = 1e-12 * (scale if scale > 0.0 else cov_scale)
        err = float(np.abs(Y - ref).max())
        print(f"{Ns} ell={ell} theta={theta} kind={kind} {param}: err / bar = {err / bar:.3e}")
        _record(f"{lm.KINDS[kind]} {param}", err / bar)
        assert err <= bar, (param, err, bar)
        if param in ("log_ell0", "log_ell1", "log_ell2"):
            per_axis += Y
        if param == "log_ell":
            total = Y
    # log_ell is the sum of the per-axis derivatives, each product within the bar
    tref = float(np.abs(total).max())
    assert np.abs(total - per_axis).max() <= (1 + len(Ns)) * 1e-12 * max(tref, 1e-300) or tref == 0.0


@pytest.mark.parametrize("kind", range(4))
def test_theta_with_equal_lengths_is_zero(gsi, ctx, kind):
    op = gsi.fft_gridcov_derivative(ctx, [7, 5], "theta", kind=lm.KINDS[kind], ell=[2.0, 2.0], theta=0.4, sigma2=SIGMA2)
    try:
        Y = _columns(op)
    finally:
        op.close()
    assert np.abs(Y).max() <= 1e-12 * SIGMA2


@pytest.mark.parametrize("kind", range(4))
@pytest.mark.parametrize("Ns,ell,theta", [((7, 5), (3.0, 1.5), 0.0), ((7, 5), (3.0, 1.5), 0.4), ((3, 4, 5), (3.0, 2.0, 4.0), 0.0)])
def test_log_sigma2_has_the_bits_of_the_covariance_operator(gsi, ctx, Ns, ell, theta, kind):
    X = np.random.default_rng(int(np.prod(Ns)) + kind).standard_normal((int(np.prod(Ns)), 6))
    a = gsi.fft_gridcov_derivative(ctx, Ns, "log_sigma2", kind=lm.KINDS[kind], ell=ell, theta=theta, sigma2=SIGMA2)
    b = gsi.fft_gridcov_operator(ctx, Ns, kind=lm.KINDS[kind], ell=ell, theta=theta, sigma2=SIGMA2, nugget=0.0)
    try:
        assert np.array_equal(a.matmul(X), b.matmul(X))
    finally:
        a.close()
        b.close()


def test_refusals(gsi, ctx):
    before = ctx.device_bytes()
    for kw, word in ((dict(Ns=[8, 6], param=7), "param"), (dict(Ns=[8, 6], param=-1), "param"),
                     (dict(Ns=[12], param="theta"), "THETA"), (dict(Ns=[4, 5, 6], param="theta"), "THETA"),
                     (dict(Ns=[12], param="log_ell1"), "LOG_ELL"), (dict(Ns=[8, 6], param="log_ell2"), "LOG_ELL"),
                     (dict(Ns=[8, 6], param="log_ell", ell=0.0), "ell"), (dict(Ns=[8, 6], param="log_ell", sigma2=-1.0), "sigma2"),
                     (dict(Ns=[8, 6], param="log_ell", kind=4), "kind"), (dict(Ns=[4, 5, 6], param="log_ell", theta=0.3), "theta"),
                     (dict(Ns=[5000], param="log_ell"), "4096 grid points per axis"),
                     (dict(Ns=[1024, 512, 512], param="log_ell", ell=10.0), "fewer than 2^31")):
        kw = dict(kw)
        Ns, param = kw.pop("Ns"), kw.pop("param")
        sc.refused(gsi, lambda: gsi.fft_gridcov_derivative(ctx, Ns, param, **kw), word)
    assert ctx.device_bytes() == before


# ---- through fft_operator_at and linear_data_operator ------------------------------------------------------------------------
AT_NS, AT_M, AT_ELL, AT_THETA = (12, 9), 40, (3.0, 2.0), 0.3


def _at_dense(param, kind):
    P = im.scattered_points(AT_NS, AT_M, seed=19)
    box = im.inner_box(P, shrink=0.05)
    base, frac = im.plan(P, AT_NS, box)
    W = am.weights_matrix(AT_NS, base, frac)
    dC = lm.dk_entries(AT_NS, kind, AT_ELL, AT_THETA, SIGMA2, param).astype(np.float64)
    return P, box, W @ dC @ W.T


@pytest.mark.parametrize("kind", [1, 3])
def test_through_the_points_operator_and_the_linear_data_operator(gsi, ctx, kind):
    for param in ("log_sigma2", "log_ell", "log_ell0", "log_ell1", "theta", "nugget"):
        P, box, A = _at_dense(param, kind)
        gop = gsi.fft_gridcov_derivative(ctx, AT_NS, param, kind=lm.KINDS[kind], ell=AT_ELL, theta=AT_THETA, sigma2=SIGMA2)
        op = gsi.fft_operator_at(ctx, gop, P, box=box)
        try:
            Y = op.matmul(np.eye(AT_M))
            _record("W dC W' ratio", fc.close(Y, A, f"W dC W' {lm.KINDS[kind]} {param}"))
        finally:
            op.close()
        # 20 rows of a sparse H over the same grid
        n = int(np.prod(AT_NS))
        H = np.zeros((20, n))
        rng = np.random.default_rng([7, kind])
        indptr, indices, data = [0], [], []
        for r in range(20):
            cols = np.sort(rng.choice(n, size=5, replace=False))
            vals = rng.standard_normal(5)
            H[r, cols] = vals
            indices += cols.tolist()
            data += vals.tolist()
            indptr.append(len(indices))
        mdl = gsi.LinearForwardModel((np.array(indptr), np.array(indices), np.array(data), (20, n)), link="identity", ctx=ctx)
        hop = gsi.linear_data_operator(gop, mdl)
        try:
            dC = lm.dk_entries(AT_NS, kind, AT_ELL, AT_THETA, SIGMA2, param).astype(np.float64)
            _record("H dC H' ratio", fc.close(hop.matmul(np.eye(20)), H @ dC @ H.T, f"H dC H' {lm.KINDS[kind]} {param}"))
        finally:
            hop.close()
            mdl.close()
            gop.close()


# ---- the shared points plan ----------------------------------------------------------------------------------------------
def test_like_product_has_the_bits_of_a_freshly_planned_operator(gsi, ctx):
    P = im.scattered_points(AT_NS, AT_M, seed=19)
    box = im.inner_box(P, shrink=0.05)
    X = np.random.default_rng(2).standard_normal((AT_M, 7))
    g1 = gsi.fft_gridcov_operator(ctx, AT_NS, kind="exponential", ell=AT_ELL, theta=AT_THETA)
    g2 = gsi.fft_gridcov_derivative(ctx, AT_NS, "log_ell", kind="exponential", ell=AT_ELL, theta=AT_THETA)
    base = gsi.fft_operator_at(ctx, g1, P, box=box)
    fresh = gsi.fft_operator_at(ctx, g2, P, box=box)
    before = ctx.device_bytes()
    like = gsi.fft_operator_at(ctx, g2, like=base)
    try:
        assert ctx.device_bytes() == before                     # nothing planned, nothing uploaded
        assert like.shape == (AT_M, AT_M) and like.Ns == AT_NS and np.array_equal(like.steps, base.steps)
        assert np.array_equal(like.matmul(X), fresh.matmul(X))
        like2 = gsi.fft_operator_at(ctx, g1, like=like)        # a like operator serves as `like` itself
        assert np.array_equal(like2.matmul(X), base.matmul(X))
        like2.close()
    finally:
        for h in (like, fresh, base, g1, g2):
            h.close()


def test_destruction_in_every_order(gsi, ctx):
    P = im.scattered_points(AT_NS, AT_M, seed=19)
    X = np.random.default_rng(3).standard_normal((AT_M, 3))
    want = None
    for order in itertools.permutations(range(4)):
        g1 = gsi.fft_gridcov_operator(ctx, AT_NS, kind="gaussian", ell=2.0)
        g2 = gsi.fft_gridcov_derivative(ctx, AT_NS, "log_ell", kind="gaussian", ell=2.0)
        base = gsi.fft_operator_at(ctx, g1, P)
        like = gsi.fft_operator_at(ctx, g2, like=base)
        hs = [g1, g2, base, like]
        Y = [base.matmul(X), like.matmul(X)]
        if want is None:
            want = Y
        for k in order[:3]:                                    # three go, in this order; the survivor still works
            hs[k].close()
        last = hs[order[3]]
        Z = last.matmul(X) if order[3] >= 2 else last.matmul(np.eye(int(np.prod(AT_NS))))
        if order[3] >= 2:
            assert np.array_equal(Z, want[order[3] - 2]), order
        else:
            assert np.isfinite(Z).all()
        last.close()


def test_like_refusals(gsi, ctx):
    P = im.scattered_points(AT_NS, AT_M, seed=19)
    g1 = gsi.fft_gridcov_operator(ctx, AT_NS, kind="gaussian", ell=2.0)
    other_shape = gsi.fft_gridcov_operator(ctx, [9, 12], kind="gaussian", ell=2.0)
    base = gsi.fft_operator_at(ctx, g1, P)
    dense = gsi.dense_operator(ctx, np.eye(AT_M))
    other = gsi.Context(0)
    try:
        sc.refused(gsi, lambda: gsi.fft_operator_at(ctx, other_shape, like=base), "same grid shape")
        sc.refused(gsi, lambda: gsi.fft_operator_at(ctx, g1, like=g1), "like must be an operator of gsi_op_fft_at")
        sc.refused(gsi, lambda: gsi.fft_operator_at(ctx, g1, like=dense), "like must be an operator of gsi_op_fft_at")
        sc.refused(gsi, lambda: gsi.fft_operator_at(ctx, dense, like=base), "FFT covariance operator")
        g_other = gsi.fft_gridcov_operator(other, AT_NS, kind="gaussian", ell=2.0)
        try:
            sc.refused(gsi, lambda: gsi.fft_operator_at(ctx, g_other, like=base), "another context")
            sc.refused(gsi, lambda: gsi.fft_operator_at(other, g_other, like=base), "another context")
        finally:
            g_other.close()
        with pytest.raises(ValueError):
            gsi.fft_operator_at(ctx, g1, P, like=base)
        with pytest.raises(ValueError):
            gsi.fft_operator_at(ctx, g1)
    finally:
        other.close()
        for h in (dense, base, other_shape, g1):
            h.close()
