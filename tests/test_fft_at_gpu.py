"""FFT covariance operators at scattered points on the GPU: the spread W' X (csrc/interp_adjoint.hip, `gsi_fftrf_spread`) and the
operator W C W' (`gsi_op_fft_at`, `fft_operator_at`); DESIGN.md 4.6g.

Bounds of the spread alone (derived, not measured), against the longdouble model, per node g with k_g contributions:
    |G_dev[g, c] - G_ref[g, c]| <= (k_g + 8) 2^-53 sum_p |w(p, g)| |X[p, c]|
(k_g - 1 additions in any order or chunking: at most k_g - 1 roundings; the weight and the product: at most d + 1 more; the
rest is second-order slack), and of the adjoint identity with device gather and device spread, host dots in longdouble:
    |<W v, x> - <v, W' x>| <= (k_max + 2^d + 16) 2^-53 sum_{p, g} |x_p| |w(p, g)| |v_g|
Products through the FFT passes are held to the project's bar for them, err < 1e-12 max|Y_ref| (test_fft_gridcov_gpu._close).
`FFT_AT_ERRORS=<path>`: the measured ratios of tests 1, 5 and 7 are written there as JSON (profiles/fft_at_errors.json)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import fftrf_interp_model as im
import interp_adjoint_model as am
from helpers import rel_sv_err
from oracle import oracle as orc
from test_fft_gridcov_cpu import dense_matrix
from test_fft_gridcov_gpu import _close

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the planner's chunk limit, from its header
CHUNK = int(re.search(r"IADJ_CHUNK\s*=\s*(\d+)", open(os.path.join(ROOT, "geostatinversion.jl_amd", "csrc",
                                                                  "interp_adjoint_plan.hpp")).read()).group(1))
RATIOS = {}
BARS = {"spread_err_over_bound": "|G_dev - G_longdouble| <= (k_g + 8) 2^-53 sum_p |w| |x| per node and column (test 1 and 2)",
        "operator_err_over_1e-12_scale": "max |Y - W C W' X| <= 1e-12 max |Y_ref| (test 5)",
        "randsvd_sv_err_over_1e-9": "helpers.rel_sv_err against the oracle's randsvd of the dense W C W' <= 1e-9 (test 7)",
        "randsvd_xis_err_over_1e-6": "oracle.xis_error_up_to_sign <= 1e-6 (test 7)"}


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()
    path = os.environ.get("FFT_AT_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump({"bars": BARS, "largest_ratio_to_its_bar": RATIOS}, f, indent=1, sort_keys=True)
            f.write("\n")


def _record(key, value):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(value))


def _spread(gsi, ctx, P, X, Ns, box=None):
    """`gsi_fftrf_spread` into a matrix filled with NaN beforehand: every entry must be written."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    n = int(np.prod(Ns))
    Xd = gsi.DeviceMatrix.from_host(ctx, X)
    G = gsi.DeviceMatrix.from_host(ctx, np.full((n, X.shape[1]), np.nan))
    try:
        arr = (C.c_int64 * len(Ns))(*Ns)
        Pf = np.asfortranarray(P, dtype=np.float64)
        bp = gsi._lib.dptr(np.ascontiguousarray(box, dtype=np.float64)) if box is not None else None
        gsi._lib.check(ctx.lib.gsi_fftrf_spread(ctx.h, G.h, Xd.h, len(Ns), arr, gsi._lib.dptr(Pf), Pf.shape[1], bp, 0), ctx.lib)
        return G.to_host()
    finally:
        Xd.close()
        G.close()


def _check_spread(G, X, Ns, base, frac, what):
    ref = am.spread(X, Ns, base, frac)
    scale = am.spread(X, Ns, base, frac, absolute=True)
    k = am.node_counts(base, Ns)
    assert np.isfinite(G).all(), what
    assert (G[k == 0] == 0.0).all() and not np.signbit(G[k == 0]).any(), what       # untouched nodes: exactly +0.0
    err = np.abs(G.astype(np.longdouble) - ref)
    bound = (k[:, None] + 8) * EPS * scale
    ratio = float((err[scale > 0] / bound[scale > 0]).max()) if (scale > 0).any() else 0.0
    print(f"{what}: max err / bound = {ratio:.3f}")
    _record("spread_err_over_bound", ratio)
    assert (err <= bound).all(), (what, ratio)
    return ratio


# ---- 1. the spread against the model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns", im.GRIDS, ids=im.gid)
def test_spread_against_the_model(gsi, ctx, Ns):
    for m in im.POINT_COUNTS:
        P = im.scattered_points(Ns, m, seed=11)
        X = np.random.default_rng([m, 5]).standard_normal((m, max(im.FIELD_COUNTS)))
        for box in [im.inner_box(P)] + ([None] if m >= 2 else []):
            base, frac = im.plan(P, Ns, box)
            for nf in im.FIELD_COUNTS:
                G = _spread(gsi, ctx, P, X[:, :nf], Ns, box)
                assert G.shape == (int(np.prod(Ns)), nf)
                _check_spread(G, X[:, :nf], Ns, base, frac, f"{im.gid(Ns)} m={m} nf={nf} box={box is not None}")


def test_one_point_leaves_every_other_node_exactly_zero(gsi, ctx):
    Ns = (33, 2, 17)
    P = np.array([[0.37], [0.81], [0.55]])
    box = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    G = _spread(gsi, ctx, P, np.array([[2.5]]), Ns, box)
    base, frac = im.plan(P, Ns, box)
    touched = base[0] + am.corner_offsets(Ns)
    mask = np.ones(G.shape[0], dtype=bool)
    mask[touched] = False
    assert (G[mask] == 0.0).all() and (G[touched] != 0.0).all()
    _check_spread(G, np.array([[2.5]]), Ns, base, frac, "one point")
    # the Python entry point returns the same bits
    D = gsi.FFTRF.spread(ctx, P, np.array([[2.5]]), Ns, box=box)
    assert np.array_equal(D.to_host(), G)
    D.close()


# ---- 2. skew -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns", [(25, 37), (6, 4, 5)], ids=im.gid)
def test_spread_with_skewed_points(gsi, ctx, Ns):
    d = len(Ns)
    rng = np.random.default_rng(17)
    m = 3 * CHUNK + 7
    box = np.concatenate([np.zeros(d), np.array(Ns, dtype=float) - 1.0])
    cell = np.array([3.0, 2.0, 1.0][:d])[:, None]
    # all m points in one cell: every node of it has at least 3 chunks and a remainder
    P = cell + 0.05 + 0.9 * rng.random((d, m))
    X = rng.standard_normal((m, 3))
    base, frac = im.plan(P, Ns, box)
    assert am.node_counts(base, Ns).max() == m and len(set(base)) == 1
    _check_spread(_spread(gsi, ctx, P, X, Ns, box), X, Ns, base, frac, f"{im.gid(Ns)} one cell")
    # half of the points in one cell, the rest uniform over the box (and beyond it: clamped onto the boundary)
    m2 = 1000
    Q = (np.array(Ns, dtype=float)[:, None] + 1.0) * rng.random((d, m2)) - 1.0
    Q[:, ::2] = cell + 0.05 + 0.9 * rng.random((d, m2 // 2))
    X2 = rng.standard_normal((m2, 7))
    base, frac = im.plan(Q, Ns, box)
    k = am.node_counts(base, Ns)
    assert k.max() >= 500 and ((k > 0) & (k <= CHUNK)).any()            # long lists beside short ones ...
    assert (k == 0).any() or k.size < m2                               # ... and, where the grid has room, empty ones
    _check_spread(_spread(gsi, ctx, Q, X2, Ns, box), X2, Ns, base, frac, f"{im.gid(Ns)} half in one cell")


# ---- 3. determinism and independence of the launch ---------------------------------------------------------------------
def test_spread_is_deterministic_and_a_column_does_not_depend_on_the_others(gsi, ctx):
    Ns, m = (25, 37), 1000
    rng = np.random.default_rng(23)
    P = im.scattered_points(Ns, m, seed=4)
    P[:, 100:100 + 4 * CHUNK] = P[:, [7]] + 1e-3 * rng.random((2, 4 * CHUNK))     # long lists as well
    X = rng.standard_normal((m, 7))
    G1 = _spread(gsi, ctx, P, X, Ns)
    G2 = _spread(gsi, ctx, P, X, Ns)
    assert np.array_equal(G1, G2)
    for c in (0, 3, 6):
        assert np.array_equal(_spread(gsi, ctx, P, X[:, [c]], Ns)[:, 0], G1[:, c]), c
    X9 = np.hstack([X, rng.standard_normal((m, 2))])              # 9 columns: a full group of 8 and a tail of one
    assert np.array_equal(_spread(gsi, ctx, P, X9, Ns)[:, :7], G1)


# ---- 4. the adjoint identity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns", [(3, 5), (25, 37), (6, 4, 5)], ids=im.gid)
def test_adjoint_identity(gsi, ctx, Ns):
    m, d = 257, len(Ns)
    rng = np.random.default_rng(29)
    P = im.scattered_points(Ns, m, seed=13)
    box = im.inner_box(P)
    v = rng.standard_normal((int(np.prod(Ns)), 1))
    x = rng.standard_normal((m, 1))
    Wv = gsi.FFTRF.interpolate(ctx, P, v, Ns, box=box)
    Wtx = _spread(gsi, ctx, P, x, Ns, box)
    lhs = np.dot(Wv.to_host()[:, 0].astype(np.longdouble), x[:, 0].astype(np.longdouble))
    Wv.close()
    rhs = np.dot(v[:, 0].astype(np.longdouble), Wtx[:, 0].astype(np.longdouble))
    base, frac = im.plan(P, Ns, box)
    kmax = am.node_counts(base, Ns).max()
    scale = np.dot(np.abs(v[:, 0]).astype(np.longdouble), am.spread(x, Ns, base, frac, absolute=True)[:, 0])
    bound = (kmax + (1 << d) + 16) * EPS * scale
    print(f"{im.gid(Ns)}: |<Wv, x> - <v, W'x>| / bound = {float(abs(lhs - rhs) / bound):.3f}")
    assert abs(lhs - rhs) <= bound


# ---- 5. the operator against the dense matrix --------------------------------------------------------------------------
def _table_case():
    Ns = (8, 6)
    t = np.exp(-np.hypot(*np.meshgrid(np.arange(8.0), np.arange(6.0), indexing="ij")) / 3.0)
    idx = np.unravel_index(np.arange(48), Ns, order="F")
    Cm = t[np.abs(idx[0][:, None] - idx[0][None, :]), np.abs(idx[1][:, None] - idx[1][None, :])] + 0.02 * np.eye(48)
    return Ns, dict(table=t, nugget=0.02), Cm


def _grid_cases(gsi, ctx):
    """(name, Ns, grid operator, dense C)"""
    out = []
    for name, Ns, kind, k, ell, theta, s2, nug in (("exp-rot", (25, 37), "exponential", 1, (6.0, 2.5), 0.6, 1.7, 0.01),
                                                   ("gauss-3d", (6, 4, 5), "gaussian", 0, (2.0, 1.5, 2.5), 0.0, 1.0, 0.0),
                                                   ("matern32-2x2", (2, 2), "matern32", 2, (1.5, 1.5), 0.0, 1.0, 0.0)):
        op = gsi.fft_gridcov_operator(ctx, list(Ns), kind=kind, ell=list(ell), theta=theta, sigma2=s2, nugget=nug)
        out.append((name, Ns, op, dense_matrix(Ns, k, ell, theta, s2, nug)))
    Ns, kw, Cm = _table_case()
    out.append(("table", Ns, gsi.fft_gridcov_operator(ctx, list(Ns), **kw), Cm))
    for fftrf in (False, True):
        op = gsi.fft_powerlaw_operator(ctx, [12, 10], -3.5, fftrf=fftrf)
        out.append((f"powerlaw-fftrf={fftrf}", (12, 10), op, op.matmul(np.eye(120))))       # existing code, not under test here
    return out


@pytest.fixture(scope="module")
def grid_cases(gsi, ctx):
    cases = _grid_cases(gsi, ctx)
    yield cases
    for _, _, op, _ in cases:
        op.close()


@pytest.mark.parametrize("m", [63, 257, 1000])
def test_operator_against_the_dense_matrix(gsi, ctx, grid_cases, m):
    rng = np.random.default_rng([31, m])
    for name, Ns, gop, Cm in grid_cases:
        P = im.scattered_points(Ns, m, seed=19)
        box = im.inner_box(P, shrink=0.05)
        base, frac = im.plan(P, Ns, box)
        W = am.weights_matrix(Ns, base, frac)
        A = W @ Cm @ W.T
        op = gsi.fft_operator_at(ctx, gop, P, box=box)
        try:
            assert op.shape == (m, m) and op.size(1) == m and op.grid_op is gop
            lo, hi = im.extent(P, box)
            assert np.array_equal(op.steps, (hi - lo) / (np.array(Ns) - 1.0))
            for l in (1, 7, 160):
                X = rng.standard_normal((m, l))
                Yref = A @ X
                Y = op.matmul(X)
                _close(Y, Yref, f"{name} m={m} l={l} A X")
                _close(op.rmatmul_t(X), Yref, f"{name} m={m} l={l} A' X")
                _record("operator_err_over_1e-12_scale", np.abs(Y - Yref).max() / np.abs(Yref).max() / 1e-12)
            if m <= 257:
                Ad = op.matmul(np.eye(m))
                assert np.abs(Ad - Ad.T).max() <= 1e-12 * np.abs(A).max(), name
            dg = op.diagonal()
            assert np.abs(dg - np.diag(A)).max() <= 1e-12 * np.abs(A).max(), name
        finally:
            op.close()


# ---- 6. column batches -------------------------------------------------------------------------------------------------
def test_column_batches(gsi, ctx, grid_cases, monkeypatch):
    name, Ns, gop, Cm = grid_cases[0]
    m, l = 257, 7
    P = im.scattered_points(Ns, m, seed=37)
    base, frac = im.plan(P, Ns)
    W = am.weights_matrix(Ns, base, frac)
    X = np.random.default_rng(41).standard_normal((m, l))
    Yref = W @ (Cm @ (W.T @ X))
    op = gsi.fft_operator_at(ctx, gop, P)
    try:
        monkeypatch.delenv("GSI_FFT_AT_BATCH", raising=False)
        results = {"default": op.matmul(X)}
        for b in ("2", "4"):
            monkeypatch.setenv("GSI_FFT_AT_BATCH", b)
            results[b] = op.matmul(X)
            assert np.array_equal(op.matmul(X), results[b]), b           # repeated calls at one setting: identical bits
        monkeypatch.delenv("GSI_FFT_AT_BATCH")
        assert np.array_equal(op.matmul(X), results["default"])
        for b, Y in results.items():
            _close(Y, Yref, f"batch {b}")
    finally:
        op.close()


# ---- 7. randsvd and the xi-basis ---------------------------------------------------------------------------------------
def test_randsvd_and_the_xi_basis(gsi, ctx):
    Ns, m, K, p, q = (25, 37), 600, 20, 10, 2
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=[6.0, 6.0])
    P = im.scattered_points(Ns, m, seed=43)
    base, frac = im.plan(P, Ns)
    W = am.weights_matrix(Ns, base, frac)
    A = W @ dense_matrix(Ns, 1, (6.0, 6.0), 0.0, 1.0, 0.0) @ W.T
    A = 0.5 * (A + A.T)
    Om = np.random.default_rng(47).standard_normal((m, K + p))
    op = gsi.fft_operator_at(ctx, gop, P)
    try:
        Z, S = gsi.randsvd(op, K, p, q, Omega=Om, return_S=True)
        Zr, Sr, _ = orc.randsvd_full(A, K, p, q, Om)
        sv, xe = rel_sv_err(S, Sr, K), orc.xis_error_up_to_sign(Z, Zr, K)
        print(f"randsvd at points: sv rel-err {sv:.2e}, xis err {xe:.2e}")
        _record("randsvd_sv_err_over_1e-9", sv / 1e-9)
        _record("randsvd_xis_err_over_1e-6", xe / 1e-6)
        assert sv < 1e-9 and xe < 1e-6
        basis = gsi.getxis_device(op, K, p, q, Omega=Om)
        assert isinstance(basis, gsi.DeviceBasis) and len(basis[0]) == m
    finally:
        op.close()
        gop.close()


# ---- 8. it is the covariance of what the sampler produces --------------------------------------------------------------
def test_operator_is_the_covariance_of_the_sampled_fields(gsi, ctx):
    """Entrywise within 6 sqrt(2 / N) (sigma2 + nugget): an entry's Monte-Carlo standard deviation is at most sqrt(2 / N) sigma2,
    so this is a 6-sigma condition on 1600 entries.  The noise comes from numpy (interp_adjoint_model.SAMPLER_SEED), so the
    model (gridcov_sample_model.fields_from_eps) sees the same fields on the CPU, where
    test_interp_adjoint_model.test_sampler_seed_stays_inside_the_monte_carlo_bound confirms the bound for that seed."""
    Ns, P, box = am.sampler_case()
    smp = gsi.gridcov_sampler(ctx, list(Ns), kind="exponential", ell=6.0, embed="auto")
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=6.0)
    op = gsi.fft_operator_at(ctx, gop, P, box=box)
    try:
        assert smp.M == (64, 64)                          # the torus of the CPU confirmation
        F = smp.fields(am.SAMPLER_N, eps=am.sampler_noise(smp.Mtot))
        V = gsi.FFTRF.interpolate(ctx, P, F, Ns, box=box)
        F.close()
        Vh = V.to_host()
        V.close()
        emp = Vh @ Vh.T / am.SAMPLER_N                       # about the known zero mean
        A = op.matmul(np.eye(40))
        ratio = np.abs(emp - A).max() / am.sampler_bound()
        print(f"sampled covariance against the operator: max err / bound = {ratio:.3f}")
        assert ratio <= 1.0
    finally:
        op.close()
        gop.close()
        smp.close()


# ---- 9. refusals and lifetimes -----------------------------------------------------------------------------------------
def _refused(gsi, fn, word):
    with pytest.raises(gsi.GsiError) as ei:
        fn()
    assert ei.value.code == 1 and word in str(ei.value), ei.value


def test_refusals(gsi, ctx, monkeypatch):
    Ns = (9, 7)
    P = im.scattered_points(Ns, 50, seed=3)
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="gaussian", ell=2.0)
    try:
        dense = gsi.dense_operator(ctx, np.eye(63))
        _refused(gsi, lambda: gsi.fft_operator_at(ctx, dense, P), "FFT covariance operator")
        dense.close()
        line = gsi.fft_gridcov_operator(ctx, [50], kind="exponential", ell=7.0)
        _refused(gsi, lambda: gsi.fft_operator_at(ctx, line, P[:1]), "2 or 3 axes")
        line.close()
        flat = gsi.fft_gridcov_operator(ctx, [1, 50], kind="exponential", ell=7.0)
        _refused(gsi, lambda: gsi.fft_operator_at(ctx, flat, P), "N[a] >= 2")
        flat.close()
        other = gsi.Context(0)
        try:
            _refused(gsi, lambda: gsi.fft_operator_at(other, gop, P), "another context")
        finally:
            other.close()
        for bad in (np.nan, np.inf):
            Q = P.copy()
            Q[1, 17] = bad
            _refused(gsi, lambda: gsi.fft_operator_at(ctx, gop, Q), "finite")
        Q = P.copy()
        Q[0, :] = 2.5
        _refused(gsi, lambda: gsi.fft_operator_at(ctx, gop, Q), "extent")
        _refused(gsi, lambda: gsi.fft_operator_at(ctx, gop, P, box=[0.0, 0.0, 0.0, 1.0]), "extent")
        # spread: more rows than points (the library), fewer (the wrapper)
        _refused(gsi, lambda: gsi.FFTRF.spread(ctx, P, np.zeros((51, 2)), Ns), "rows")
        with pytest.raises(ValueError):
            gsi.FFTRF.spread(ctx, P, np.zeros((49, 2)), Ns)
        # a context with a communicator (one rank, threads-of-one-process communicator)
        monkeypatch.setenv("GSI_LOCAL_COMM", "1")
        monkeypatch.setenv("GSI_FORCE_COMM", "1")
        cc = gsi.Context(0)
        try:
            cc.comm_init(1, 0, cc.unique_id())
            g2 = gsi.fft_gridcov_operator(cc, list(Ns), kind="gaussian", ell=2.0)
            _refused(gsi, lambda: gsi.fft_operator_at(cc, g2, P), "communicator")
            g2.close()
        finally:
            cc.close()
    finally:
        gop.close()


def test_either_order_of_destruction(gsi, ctx):
    Ns = (9, 7)
    P = im.scattered_points(Ns, 50, seed=3)
    X = np.random.default_rng(1).standard_normal((50, 3))
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="gaussian", ell=2.0)
    op = gsi.fft_operator_at(ctx, gop, P)
    Y = op.matmul(X)                              # (a first cycle: whatever workspace the products cache exists from here on)
    op.close()
    gop.close()
    ctx.release_cache()
    before = ctx.device_bytes()
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="gaussian", ell=2.0)
    op = gsi.fft_operator_at(ctx, gop, P)
    assert np.array_equal(op.matmul(X), Y)
    gop.close()                                   # the grid operator first: the plan lives on in the new operator
    assert np.array_equal(op.matmul(X), Y)
    op.close()
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="gaussian", ell=2.0)
    op = gsi.fft_operator_at(ctx, gop, P)
    op.close()                                    # the reverse order: the grid operator still works
    Z = gop.matmul(np.eye(63))
    assert np.isfinite(Z).all()
    gop.close()
    ctx.release_cache()
    assert ctx.device_bytes() == before           # plan, points plan and inverted index: all returned
