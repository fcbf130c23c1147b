"""The case table of the contraction-kernel tests (tests/gemm_cases.py), checked without a GPU: its axes are complete, its
exact cases are exact, and its checks accept a correct product and reject a wrong one -- run against a numpy stand-in for
gsi_gemm_view that lays the operands out as the library does (NaN padding, the whole C image there and back)."""
import numpy as np
import pytest

import gemm_cases as gc

SMALL_GROUPS = [g for g in gc.GROUPS if g not in gc.BIG_GROUPS]


def host_gemm_view(A, B, C_image, *, m, l, k, form=0, trans=False, alpha=1.0, beta=0.0, lda, a_off=0, ldb=0, b_off=0, ldc,
                   c_off=0, m_full=0, r0=0, wrong=None):
    """What gsi_gemm_view computes, in numpy, through the same strided device images."""
    tn = trans or form == 1
    ar, ac = (m_full, k) if form == 3 else ((k, m) if tn else (m, k))
    Ad = np.full(a_off + lda * ac, np.nan)
    Ad[a_off:].reshape((lda, ac), order="F")[:ar] = A
    Av = Ad[a_off:].reshape((lda, ac), order="F")[:ar]
    if form == 1:
        Bv = Av
    else:
        Bd = np.full(b_off + ldb * l, np.nan)
        Bd[b_off:].reshape((ldb, l), order="F")[:k] = B
        Bv = Bd[b_off:].reshape((ldb, l), order="F")[:k]
    img = np.array(C_image, dtype=np.float64)
    Cv = img[c_off:c_off + ldc * l].reshape((ldc, l), order="F")
    opA = Av.T if tn else Av[r0:r0 + m]
    P = alpha * (opA @ Bv)
    if wrong == "entry":
        P[m // 2, l // 3] += 1.0
    if wrong == "stale-c":
        P = P + 0.0 * Cv[r0:r0 + m]
    Cv[r0:r0 + m] = P + (beta * Cv[r0:r0 + m] if beta != 0.0 else 0.0)
    if wrong == "spill":
        img[c_off + m if ldc > m else 0] = 0.25          # a store one row below the view
    return img, None


def test_ids_are_unique_and_axes_complete():
    cases = gc.all_cases()
    assert len({c.id for c in cases}) == len(cases)
    for trans in (False, True):
        mine = [c for c in cases if c.form == 0 and c.trans == trans]
        assert {c.m for c in mine} >= set(gc.M_AXIS)
        assert {c.k for c in mine} >= set(gc.K_AXIS)
        assert {(c.alpha, c.beta) for c in mine if not c.real} >= set(gc.AB)
        for which in ("a", "b", "c"):            # each operand: odd offset alone, odd leading dimension alone, both
            seen = {(getattr(c, which + "_off") & 1, getattr(c, "LD" + which.upper()) & 1) for c in mine if c.group == "align"}
            assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {c.l for c in mine if c.group == "nt"} == {v for nt in range(1, 11) for v in (16 * nt, 16 * nt - 1, 16 * nt - 15)}
        # TN with K odd: the 16-byte path with a partial last tile (lda even) and the element-wise path (lda odd)
        if trans:
            assert {c.LDA & 1 for c in mine if c.group == "rows" and c.k & 1} == {0, 1}
    assert {g for g in gc.GROUPS} == {c.group for c in cases}
    assert all(any(c.real for c in gc.group_cases(g)) for g in gc.GROUPS)


def test_exact_cases_are_exact_in_any_order():
    """|partial sums| <= 16 K, alpha a power of two times +-1, |beta C0| <= 16: everything is a multiple of 1/2 below 2^53."""
    for c in gc.all_cases():
        if not c.real:
            assert c.alpha in gc.ALPHAS and c.beta in gc.BETAS
            assert 2 * (16 * c.k + 16) < 2 ** 53


def test_footprints():
    """Outside the persistent and large-leading-dimension groups a case uploads a few MB at most."""
    for c in gc.all_cases():
        host = 8 * (c.a_rows * c.a_cols + c.k * c.l + 2 * c.image_doubles)
        if c.group not in gc.BIG_GROUPS:
            assert host < 48e6, c.id
        assert 8 * (c.a_off + c.LDA * c.a_cols) < 4.4e9 and 8 * (c.b_off + c.LDB * c.l) < 4.4e9, c.id


@pytest.mark.parametrize("group", SMALL_GROUPS)
def test_checks_accept_a_host_product(group):
    for case in gc.group_cases(group):
        img0, img, plan, ops = gc.run_case(host_gemm_view, case)
        bad, ratio = gc.check_case(case, img0, img, plan, ops)
        assert not bad, (case.id, bad)
        assert (ratio is not None) == case.real
        if case.real:
            assert ratio < 1.0


@pytest.mark.parametrize("wrong", ["entry", "stale-c", "spill"])
def test_checks_reject_a_wrong_product(wrong):
    import functools
    hits = 0
    for case in gc.group_cases("align")[:24]:
        if case.real or (wrong == "stale-c" and case.beta != 0.0):
            continue
        img0, img, plan, ops = gc.run_case(functools.partial(host_gemm_view, wrong=wrong), case)
        bad, _ = gc.check_case(case, img0, img, plan, ops)
        assert bad, (wrong, case.id)
        hits += 1
    assert hits >= 5
