"""The table of tests/householder_qr_cases.py sees what it claims: the numpy restatement of the Householder tier
(tests/householder_qr_model.py) passes every case, and each planted defect fails exactly the cases named here.  Every case
of the table is failed by at least one defect: a case that no defect can fail would show nothing."""
import numpy as np
import pytest

import householder_qr_cases as hc
import householder_qr_model as hm

ALL_FULL = hc.FORCED + hc.GATE + hc.RANKDEF
SCALE_NAMES = ["scale%+d" % s for s in hc.SCALINGS]
RANGE_NAMES = ["range%+d" % s for s in hc.RANGES]
EVERY_NAME = [c.name for c in ALL_FULL] + hc.EXACT + SCALE_NAMES + RANGE_NAMES

# defect -> the cases that fail under it, and why the others do not
FAILS = {
    # more than 16 workgroups at j = 0: m - j > 4096
    "no_second_trip": {"4400x20", "262145x17", "4400x20graded"},
    # rows_per_thread > 1: m > 262144
    "one_sweep": {"262145x17"},
    # every case with a row below the diagonal that holds something: not 1 x 1, and not the exact cases, whose dropped rows
    # are zero ([U; 0]) or whose +-1 entries the dropped rows miss
    "drop_last_row": set(EVERY_NAME) - {"1x1"} - set(hc.EXACT),
    # a trailing update exists (l > 16) and T is not symmetric; the scaling cases compare two runs with the same wrong T
    "T_not_transposed": {"17x17", "33x32", "300x17", "257x31", "513x33", "4400x20", "262145x17", "300x41graded",
                         "4400x20graded", "100x60", "1100x1025", "2000x40rank7", "2000x40rank7zerocol", "signed40x20"}
                        | set(RANGE_NAMES),
    # the last column of the last panel is left as it was: invisible where it has no rows below the diagonal that matter
    # (1 x 1, 17 x 17), where it is rounding noise (the rank-7 panels), where it is zero below the diagonal ([U; 0]), and in
    # the scaling cases (both runs leave it alone)
    "nlive_short": set(EVERY_NAME) - {"1x1", "17x17", "2000x40rank7", "2000x40rank7zerocol", "upper40x20"} - set(SCALE_NAMES),
    # the cases that take the sigma == 0 branch: m == l (the last reflector), the zero column, [U; 0]
    "stale_tau": {"1x1", "5x5", "16x16", "17x17", "2000x40rank7zerocol", "upper40x20"},
    "no_prescale": set(RANGE_NAMES),
}


def failing_cases(qr):
    bad = set()
    for c in ALL_FULL:
        ref = hc.reference(c)
        Q, R = qr(ref["Y"].copy(order="F"))
        if hc.failed(hc.measure(ref["Y"], Q, R, ref, rank_deficient=c in hc.RANKDEF)):
            bad.add(c.name)
    for name in hc.EXACT:
        if hc.exact_failed(qr, name):
            bad.add(name)
    for s in hc.SCALINGS:
        try:
            hc.check_scaling(qr, s)
        except AssertionError:
            bad.add("scale%+d" % s)
    for s in hc.RANGES:
        if hc.failed(hc.range_ratios(qr, s, ())):
            bad.add("range%+d" % s)
    return bad


def model_qr(Y):
    return hm.qr(Y)[:2]


@pytest.mark.parametrize("case", ALL_FULL, ids=lambda c: c.name)
def test_model_passes_table(case):
    hc.check_case(model_qr, case, who="model")


@pytest.mark.parametrize("name", hc.EXACT)
def test_model_exact(name):
    hc.check_exact(model_qr, name)


def test_model_scaling_and_range():
    Y = hc.reference(hc.SCALE_BASE)["Y"]
    base = model_qr(Y.copy(order="F"))
    for s in hc.SCALINGS:
        hc.check_scaling(model_qr, s, base=base)
    for s in hc.RANGES:
        assert hc.check_range(model_qr, s, (), who="model") is not None


def test_model_tau_is_the_references():
    """tau is pinned too: a wrong tau with a consistent Q and R is what the R and Q references exist to catch."""
    for case in (c for c in hc.FORCED if c.m <= 4400):
        Y = hc.reference(case)["Y"]
        tau = hm.qr(Y)[2]
        tau_ref = hc.reference_qr(Y)[2].astype(np.float64)
        assert np.abs(tau - tau_ref).max() <= (case.l + 4) * hc.EPS * hc.reference(case)["kappa"], case.name


@pytest.mark.parametrize("defect", hm.DEFECTS)
def test_defect_fails_exactly_the_named_cases(defect):
    bad = failing_cases(lambda Y: hm.qr(Y, defect)[:2])
    assert bad == FAILS[defect], (defect, sorted(bad - FAILS[defect]), sorted(FAILS[defect] - bad))


def test_every_case_is_failed_by_some_defect():
    assert set(FAILS) == set(hm.DEFECTS)
    assert set().union(*FAILS.values()) == set(EVERY_NAME)


def test_part_buffer_holds_every_launch():
    """qr_max_blocks(m) workgroups of partials are what the backend carves; the first sweep (j = 0) launches the most."""
    for m in (1, 255, 256, 257, 4400, 262144, 262145, 524288, 524289, 3000001):
        rpb = hm.WG * hm.rows_per_thread(m)
        assert (m + rpb - 1) // rpb <= hm.max_blocks(m)
