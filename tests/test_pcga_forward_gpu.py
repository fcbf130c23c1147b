"""The sparse forward model on the MI355X (pcga_forward.hip): both forms and every instantiation against
numpy, exact and reproducible sums across lane, wave and segment edges, 64-bit offsets into an 18 GB basis, the inversions end to
end, and gsi_fwd_apply."""

import numpy as np
import pytest

import fwd_cases as fc

pytestmark = pytest.mark.gpu

FORM = {"lane": 1, "wave": 2}


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()


def _model(gsi, ctx, case, monkeypatch, seg=None, weights=True):
    if seg is None:
        monkeypatch.delenv("GSI_FWD_SEG", raising=False)
    else:
        monkeypatch.setenv("GSI_FWD_SEG", str(seg))
    fwd = gsi.LinearForwardModel((case["indptr"], case["indices"], case["data"], (case["nobs"], case["n"])),
                                 weights=case["w"] if weights else None, link="exp" if case["link"] else "identity", ctx=ctx)
    nseg, nsplit = fc.planned_segments(case["indptr"], seg or 16384)
    assert fwd.info()[:5] == [case["nobs"], case["n"], int(case["indptr"][-1]), nseg, nsplit]
    return fwd


def _basis(gsi, ctx, Z, K, precision):
    basis = gsi.DeviceBasis(gsi.DeviceMatrix.from_host(ctx, Z), K, precision=precision)
    return basis, np.stack([basis[i] for i in range(K)], axis=1)


@pytest.mark.parametrize("seg", [None, 64], ids=["seg-default", "seg64"])
@pytest.mark.parametrize("K", [5, 37])
@pytest.mark.parametrize("link", [0, 1])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("form", ["lane", "wave"])
def test_products_on_every_path(gsi, ctx, monkeypatch, form, precision, link, K, seg):
    case = fc.product_case(K, link)
    fwd = _model(gsi, ctx, case, monkeypatch, seg)
    if seg == 64:
        assert fwd.info()[4] == 15                                # the rows of 65, 200 and 1000 nonzeros are cut
    basis, Zs = _basis(gsi, ctx, case["Z"], K, precision)
    monkeypatch.setenv("GSI_FWD_FORM", form)
    got = basis.forward(fwd, case["s"], case["X"], case["delta"])
    ratio = fc.check_product(got, case, Zs)
    print(f"{form} fp{precision} link {link} K {K} seg {seg}: largest error / bound = {ratio:.3g}")
    info = fwd.info()
    assert info[5] == FORM[form] and info[6] == 0 and info[7] == 1
    fwd.close()
    basis.close()


def test_default_form_follows_the_row_length(gsi, ctx, monkeypatch):
    """Without GSI_FWD_FORM: point samples run one lane per output, long rays one wave per segment; GSI_FWD_HOST=1 is the
    host path, and all three agree within the bound."""
    monkeypatch.delenv("GSI_FWD_FORM", raising=False)
    monkeypatch.delenv("GSI_FWD_HOST", raising=False)
    rng = np.random.default_rng(3)
    n, K = 1000, 5
    Z, s, X = rng.standard_normal((n, K)), rng.standard_normal(n), rng.standard_normal(n)
    basis, Zs = _basis(gsi, ctx, Z, K, 64)
    for lengths, want in (([1] * 50, 1), ([500] * 50, 2)):
        indptr, indices, data = fc.csr_rows(n, lengths, rng)
        fwd = gsi.LinearForwardModel((indptr, indices, data, (len(lengths), n)), ctx=ctx)
        got = basis.forward(fwd, s, X, 0.25)
        assert fwd.info()[5:] == [want, 0, 1]
        monkeypatch.setenv("GSI_FWD_HOST", "1")
        host = basis.forward(fwd, s, X, 0.25)
        monkeypatch.delenv("GSI_FWD_HOST")
        assert fwd.info()[5:] == [3, 1, 2]
        ref, bound = fc.reference(indptr, indices, data, n, None, 0, fc.paramstorun(Zs, s, X, 0.25))
        assert np.all(np.abs(got - ref) <= bound) and np.all(np.abs(host - ref) <= bound)
        fwd.close()
    basis.close()


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_one_observation_and_the_two_ends_of_the_field(gsi, ctx, monkeypatch, form):
    monkeypatch.setenv("GSI_FWD_FORM", form)
    rng = np.random.default_rng(11)
    n, K = 1000, 5
    Z, s, X = rng.standard_normal((n, K)), rng.standard_normal(n), rng.standard_normal(n)
    w = 1.0 + 0.1 * rng.standard_normal(n)
    basis, Zs = _basis(gsi, ctx, Z, K, 64)
    P = fc.paramstorun(Zs, s, X, 0.25)
    # nobs = 1; and a model whose only nonzeros are columns 0 and n - 1
    for indptr, indices, data in ((np.array([0, 3]), np.array([7, 999, 7]), np.array([1.5, -2.0, 0.25])),
                                  (np.array([0, 1, 2, 4]), np.array([0, n - 1, n - 1, 0]), np.array([2.0, 3.0, -1.0, 4.0]))):
        fwd = gsi.LinearForwardModel((indptr, indices, data, (len(indptr) - 1, n)), weights=w, ctx=ctx)
        got = basis.forward(fwd, s, X, 0.25)
        ref, bound = fc.reference(indptr, indices, data, n, w, 0, P)
        assert np.all(np.abs(got - ref) <= bound)
        assert fwd.info()[5:] == [FORM[form], 0, 1]
        fwd.close()
    basis.close()


@pytest.fixture(scope="module")
def exact_case():
    """Small integers in H, s, X and Z, w = 1, link 0, delta = 0.5: every product and every sum is exact in fp64 (and the
    basis exact in fp32), so any summation order gives the same bits -- unless a nonzero is lost or counted twice."""
    rng = np.random.default_rng(5)
    n, K = 1000, 21
    lengths = [1000, 0, 1, 63, 64, 65, 127, 128, 129, 200, 1000, 3]
    indptr, indices, data = fc.csr_rows(n, lengths, rng, values="int")
    Z = rng.integers(-4, 5, size=(n, K)).astype(np.float64)
    s = rng.integers(-8, 9, size=n).astype(np.float64)
    X = rng.integers(-8, 9, size=n).astype(np.float64)
    H, _ = fc.dense_of(indptr, indices, data, n)
    ref = H @ fc.paramstorun(Z, s, X, 0.5)                       # exact: halves of small integers, sums far below 2^53
    return dict(n=n, K=K, nobs=len(lengths), link=0, indptr=indptr, indices=indices, data=data, w=None, Z=Z, s=s, X=X, ref=ref)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("seg", [None, 64], ids=["seg-default", "seg64"])
@pytest.mark.parametrize("form", ["lane", "wave"])
def test_exact_sums_across_lane_wave_and_segment_edges(gsi, ctx, monkeypatch, exact_case, form, seg, precision):
    case = exact_case
    fwd = _model(gsi, ctx, case, monkeypatch, seg, weights=False)
    basis, Zs = _basis(gsi, ctx, case["Z"], case["K"], precision)
    assert np.array_equal(Zs, case["Z"])
    monkeypatch.setenv("GSI_FWD_FORM", form)
    got = basis.forward(fwd, case["s"], case["X"], 0.5)
    monkeypatch.setenv("GSI_FWD_HOST", "1")
    host = basis.forward(fwd, case["s"], case["X"], 0.5)
    assert fwd.info()[5:] == [3, 1, 2]
    assert np.array_equal(host, case["ref"])
    assert np.array_equal(got, host), np.argwhere(got != host)[:5]
    fwd.close()
    basis.close()


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_two_calls_return_the_same_bits(gsi, ctx, monkeypatch, form):
    case = fc.product_case(37, 1)
    fwd = _model(gsi, ctx, case, monkeypatch, 64)
    assert fwd.info()[4] > 0
    basis, _ = _basis(gsi, ctx, case["Z"], 37, 64)
    monkeypatch.setenv("GSI_FWD_FORM", form)
    a = basis.forward(fwd, case["s"], case["X"], case["delta"])
    b = basis.forward(fwd, case["s"], case["X"], case["delta"])
    assert fwd.info()[5:] == [FORM[form], 0, 2]
    assert np.array_equal(a, b)
    assert np.array_equal(fwd.apply(case["Z"][:, :3]), fwd.apply(case["Z"][:, :3]))
    fwd.close()
    basis.close()


@pytest.fixture(scope="module")
def big(gsi, ctx):
    """n = 2^27, K = 18: columns 16 and 17 of the fp64 basis lie wholly beyond 2^31 elements.  The basis is filled on the
    device (18 GB, no host copy); only the columns checked are downloaded, one at a time, once for both forms."""
    n, K = 2 ** 27, 18
    Zmat = gsi.DeviceMatrix(ctx, n, K).randn(20240)
    basis = gsi.DeviceBasis(Zmat, K)
    rng = np.random.default_rng(8)
    near0, mid = np.arange(0, 40), np.arange(n // 2 - 20, n // 2 + 20)
    rows = [near0[:5], mid[:7], np.array([n - 1]), np.concatenate([near0, mid, [n - 1]]), np.array([0, n - 1]),
            mid[::-1], np.array([n - 1, n - 2, n - 1]), np.concatenate([[n - 1], near0[::3]])]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int64)
    data = rng.standard_normal(indices.size)
    used = np.unique(indices)
    s = np.full(n, 0.5)
    X = np.full(n, -0.25)
    w = np.ones(n)
    s[used] = rng.standard_normal(used.size)
    X[used] = rng.standard_normal(used.size)
    w[used] = 1.0 + 0.1 * rng.standard_normal(used.size)
    fwd = gsi.LinearForwardModel((indptr, indices, data, (len(rows), n)), weights=w, ctx=ctx)
    # the reference on the rows of the field that the model touches
    cols = [0, 15, 16, 17]
    Zu = np.empty((used.size, len(cols)))
    col = np.empty(n)
    for k, c in enumerate(cols):
        gsi._lib.check(ctx.lib.gsi_mat_download_col(ctx.h, Zmat.h, c, gsi._lib.dptr(col)), ctx.lib)
        Zu[:, k] = col[used]
    del col
    su, Xu = s[used], X[used]
    P = np.concatenate([su[:, None] + 0.25 * Zu, (su + 0.25 * Xu)[:, None], (su + 0.25 * su)[:, None], su[:, None]], axis=1)
    ref, bound = fc.reference(indptr, np.searchsorted(used, indices), data, used.size, w[used], 0, P)
    assert np.abs(Zu[:, 2:]).min() > 0 and np.abs(ref).min() > 0          # the columns beyond 2^31 carry data
    yield dict(K=K, basis=basis, fwd=fwd, s=s, X=X, sel=cols + [K, K + 1, K + 2], ref=ref, bound=bound)
    fwd.close()
    basis.close()
    Zmat.close()
    ctx.release_cache()


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_offsets_beyond_32_bits(gsi, ctx, monkeypatch, big, form):
    monkeypatch.setenv("GSI_FWD_FORM", form)
    before = big["fwd"].info()[7]
    got = big["basis"].forward(big["fwd"], big["s"], big["X"], 0.25)
    assert big["fwd"].info()[5:] == [FORM[form], 0, before + 1]
    err = np.abs(got[:, big["sel"]] - big["ref"])
    assert np.all(err <= big["bound"]), (err / big["bound"]).max()


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("link", [0, 1])
def test_inversions_with_the_model_match_the_host_lambda(gsi, ctx, monkeypatch, link, precision):
    monkeypatch.delenv("GSI_FWD_FORM", raising=False)
    monkeypatch.delenv("GSI_FWD_HOST", raising=False)
    monkeypatch.delenv("GSI_FWD_SEG", raising=False)
    info, _ = fc.run_inversions(gsi, ctx, link, precision)
    assert info[6] == 0 and info[7] > 0 and info[5] in (1, 2)


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_apply_with_a_padded_leading_dimension(gsi, ctx, monkeypatch, form):
    monkeypatch.setenv("GSI_FWD_FORM", form)
    case = fc.product_case(37, 1)
    fwd = _model(gsi, ctx, case, monkeypatch, 64)
    n, nobs, ldp, ldo = case["n"], case["nobs"], case["n"] + 13, case["nobs"] + 3
    buf = np.full((ldp, 3), np.nan, order="F")
    buf[:n] = case["Z"][:, :3]
    out = np.full((ldo, 3), -7.0, order="F")
    dp = gsi._lib.dptr
    gsi._lib.check(ctx.lib.gsi_fwd_apply(ctx.h, fwd.h, dp(buf), ldp, 3, dp(out), ldo), ctx.lib)
    ref, bound = fc.reference(case["indptr"], case["indices"], case["data"], n, case["w"], 1, case["Z"][:, :3])
    assert np.all(np.abs(out[:nobs] - ref) <= bound)
    assert np.all(out[nobs:] == -7.0)
    assert fwd.info()[5:] == [FORM[form], 0, 1]
    assert np.array_equal(fwd(case["Z"][:, 0]), out[:nobs, 0])
    fwd.close()
