"""The adjoint of a sparse forward model on the GPU: G = H' V (csrc/fwd_adjoint.hip, `gsi_fwd_adjoint_dev`,
`LinearForwardModel.adjoint`) and the forward product with resident operands (`gsi_fwd_apply_dev`); DESIGN.md 4.6l.

The adjoint is held to the numpy model (tests/fwd_adjoint_model.py) BIT FOR BIT: the order of every sum is the plan's, every
product and sum is rounded on its own, so there is nothing to bound.  The adjoint identity with the device's forward and
adjoint products and host dots in longdouble is bounded from the two products' own rounding bounds (derived, not measured):
    adjoint, per cell j with k_j contributions   |G - G_ref|[j] <= (k_j + 4) 2^-53 sum_t |h_t| |v_{r_t}|
    forward, per row r with nnz_r nonzeros        |y - y_ref|[r] <= 8 2^-52 (nnz_r + 8) sum_t |h_t| |g_{j_t}|   (fwd_cases.reference)
so  |<H g, v> - <g, H' v>| <= ((k_max + 4) + 16 (nnz_max + 8)) 2^-53 sum_{r, j} |v_r| |H[r, j]| |g_j|."""
import numpy as np
import pytest

import fwd_adjoint_model as fm
import fwd_cases

pytestmark = pytest.mark.gpu

CHUNK, COLS = fm.CHUNK, fm.COLS
BS = [1, COLS - 1, COLS, COLS + 1, 2 * COLS + 1]


@pytest.fixture(scope="module")
def ctx(gsi):
    return gsi.default_context()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _adjoint_into_nan(gsi, ctx, mdl, V):
    """`gsi_fwd_adjoint_dev` into a matrix filled with NaN beforehand: every entry must be written."""
    Vd = gsi.DeviceMatrix.from_host(ctx, V)
    G = gsi.DeviceMatrix.from_host(ctx, np.full((mdl.n, V.shape[1]), np.nan))
    try:
        gsi._lib.check(ctx.lib.gsi_fwd_adjoint_dev(ctx.h, mdl.h, Vd.h, G.h), ctx.lib)
        return G.to_host()
    finally:
        Vd.close()
        G.close()


@pytest.mark.parametrize("with_w", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("n", [256, 257, 1000])
def test_adjoint_equals_the_model_bit_for_bit(gsi, ctx, monkeypatch, n, with_w):
    monkeypatch.delenv("GSI_FWD_HOST", raising=False)
    indptr, indices, data, lengths = fm.fan(n)
    nobs = len(indptr) - 1
    assert nobs == 3 * CHUNK + 5 and set(fm.FAN_LENGTHS) <= set(lengths.tolist())
    w = fm.weights(n) if with_w else None
    pl = fm.plan(indptr, indices, data, n, w)
    mdl = gsi.LinearForwardModel((indptr, indices, data, (nobs, n)), weights=w, ctx=ctx)
    try:
        assert not mdl.adjoint_info()["built"] and mdl.adjoint_info()["resident_bytes"] == 0       # lazy
        V = np.random.default_rng([n, 7]).standard_normal((nobs, max(BS)))
        want = fm.adjoint(pl, V)
        for b in BS:
            G = _adjoint_into_nan(gsi, ctx, mdl, V[:, :b])
            assert np.isfinite(G).all(), b
            assert (G[lengths == 0] == 0.0).all() and not np.signbit(G[lengths == 0]).any(), b   # untouched cells: exactly +0.0
            assert _same_bits(G, want[:, :b]), (b, np.abs(G - want[:, :b]).max())
            assert _same_bits(_adjoint_into_nan(gsi, ctx, mdl, V[:, :b]), G), b                   # two calls: the same bits
        ai = mdl.adjoint_info()
        assert ai["built"] and ai["resident_bytes"] > 0 and ai["host_products"] == 0 and ai["products"] == 2 * len(BS), ai
        assert ai["long_columns"] == int((lengths > CHUNK).sum()) and ai["chunks"] == len(pl["chunk_off"])
        assert ai["longest_list"] == 3 * CHUNK + 5
        monkeypatch.setenv("GSI_FWD_HOST", "1")                                                    # the host path: the same bits
        assert _same_bits(_adjoint_into_nan(gsi, ctx, mdl, V), want)
        assert mdl.adjoint_info()["host_products"] == 1
        monkeypatch.delenv("GSI_FWD_HOST")
        assert _same_bits(mdl.adjoint(V[:, 3]), want[:, 3])                                        # the Python entry, a vector
    finally:
        mdl.close()


def test_one_observation(gsi, ctx):
    n = 257
    idx = np.array([5, 256, 5, 0], dtype=np.int64)                     # unsorted, a repeated index
    val = np.array([0.3, -1.7, 2.9, 0.11])
    mdl = gsi.LinearForwardModel((np.array([0, 4]), idx, val, (1, n)), ctx=ctx)
    try:
        V = np.random.default_rng(1).standard_normal((1, COLS + 1))
        G = _adjoint_into_nan(gsi, ctx, mdl, V)
        assert _same_bits(G, fm.adjoint(fm.plan([0, 4], idx, val, n), V))
        assert np.count_nonzero(G[:, 0]) == 3
    finally:
        mdl.close()


def test_integer_values_give_the_exact_sum(gsi, ctx):
    n = 1000
    indptr, indices, data, _ = fm.fan(n, values="int")
    nobs = len(indptr) - 1
    mdl = gsi.LinearForwardModel((indptr, indices, data, (nobs, n)), ctx=ctx)
    try:
        V = np.random.default_rng(2).integers(-8, 9, size=(nobs, COLS + 1)).astype(float)
        assert np.array_equal(_adjoint_into_nan(gsi, ctx, mdl, V), fm.dense(indptr, indices, data, n).T @ V)
    finally:
        mdl.close()


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_apply_dev_equals_apply(gsi, ctx, monkeypatch, form):
    monkeypatch.setenv("GSI_FWD_FORM", form)
    n = 1000
    indptr, indices, data, _ = fm.fan(n)
    nobs = len(indptr) - 1
    w = fm.weights(n)
    for link in ("identity", "exp"):
        mdl = gsi.LinearForwardModel((indptr, indices, data, (nobs, n)), weights=w, link=link, ctx=ctx)
        try:
            P = 0.5 * np.random.default_rng(4).standard_normal((n, 5))
            Pd = gsi.DeviceMatrix.from_host(ctx, P)
            Od = mdl.apply_dev(Pd)
            got = Od.to_host()
            Od.close()
            Pd.close()
            assert _same_bits(got, mdl.apply(P)), link                    # the same kernels, the output left on the device
            ref, bound = fwd_cases.reference(indptr, indices, data, n, w, int(link == "exp"), P)
            assert (np.abs(got - ref) <= bound).all(), link
            assert mdl.info()[5] == {"lane": 1, "wave": 2}[form] and mdl.info()[6] == 0
        finally:
            mdl.close()


@pytest.mark.parametrize("n", [257, 1000])
def test_adjoint_identity(gsi, ctx, n):
    indptr, indices, data, lengths = fm.fan(n)
    nobs = len(indptr) - 1
    w = fm.weights(n)
    mdl = gsi.LinearForwardModel((indptr, indices, data, (nobs, n)), weights=w, ctx=ctx)
    try:
        rng = np.random.default_rng(29)
        g, v = rng.standard_normal(n), rng.standard_normal(nobs)
        Hg, Htv = mdl.apply_dev(g), mdl.adjoint(v)
        lhs = np.dot(Hg.astype(fm.LD), v.astype(fm.LD))
        rhs = np.dot(g.astype(fm.LD), Htv.astype(fm.LD))
        Habs = np.abs(fm.dense(indptr, indices, np.abs(data), n, np.abs(w))).astype(fm.LD)
        scale = np.abs(v).astype(fm.LD) @ Habs @ np.abs(g).astype(fm.LD)
        bound = ((lengths.max() + 4) + 16 * (np.diff(indptr).max() + 8)) * fm.EPS * scale
        print(f"n={n}: |<Hg, v> - <g, H'v>| / bound = {float(abs(lhs - rhs) / bound):.3f}")
        assert abs(lhs - rhs) <= bound
    finally:
        mdl.close()


def test_offsets_beyond_32_bits(gsi, ctx):
    """n = 2^27 cells and b = 17 columns: G holds more than 2^31 elements.  H touches the first and the last cell; G is read
    back through `apply_dev` of a point-sample model at touched and untouched cells, so the big panel never leaves the device.
    Integer values: the sums are exact."""
    n, b = 1 << 27, 17
    mid = (1 << 26) + 12345
    idx = np.array([0, n - 1, n - 1, mid, 0, mid, n - 1], dtype=np.int64)
    val = np.array([2.0, -1.0, 4.0, 1.0, -2.0, 8.0, 1.0])
    ptr = np.array([0, 2, 4, 4, 7], dtype=np.int64)                    # 4 observations, one of them empty
    V = np.random.default_rng(3).integers(-8, 9, size=(4, b)).astype(float)
    look = np.array([0, 1, 255, 256, mid - 1, mid, mid + 1, n - 257, n - 2, n - 1], dtype=np.int64)
    H = np.zeros((4, len(look)))
    for r in range(4):
        for t in range(ptr[r], ptr[r + 1]):
            H[r, np.flatnonzero(look == idx[t])[0]] += val[t]
    mdl = gsi.LinearForwardModel((ptr, idx, val, (4, n)), ctx=ctx)
    probe = gsi.LinearForwardModel((np.arange(len(look) + 1), look, np.ones(len(look)), (len(look), n)), ctx=ctx)
    Vd = gsi.DeviceMatrix.from_host(ctx, V)
    G = gsi.DeviceMatrix(ctx, n, b)
    try:
        G.randn(1)                                                     # whatever the adjoint does not write stays nonzero
        gsi._lib.check(ctx.lib.gsi_fwd_adjoint_dev(ctx.h, mdl.h, Vd.h, G.h), ctx.lib)
        got = probe.apply_dev(G)
        try:
            assert np.array_equal(got.to_host(), H.T @ V)
        finally:
            got.close()
        assert mdl.adjoint_info()["resident_bytes"] >= 8 * (n + 1) and mdl.adjoint_info()["host_products"] == 0
    finally:
        for h in (G, Vd, probe, mdl):
            h.close()
        ctx.release_cache()
