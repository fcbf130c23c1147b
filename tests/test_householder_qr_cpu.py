"""The checks of tests/householder_qr_cases.py on numpy's LAPACK QR (dgeqrf + dorgqr: the same dlarfg convention) and on the
CPU reference library (gsio_qr_thinQ: unblocked, scaled nrm2 and hypot): the inputs and bars are shown to be fair before a
GPU sees them (tests/test_householder_qr_gpu.py runs the same checks on the HIP kernels).  Run with -s to see every ratio
measured / bar; the largest per bar are printed at the end and quoted in the GPU module's docstring."""
import numpy as np
import pytest

import cpuref
import householder_qr_cases as hc

ALL_FULL = hc.FORCED + hc.GATE + hc.RANKDEF

# The one bar a yardstick misses: the CPU library sums its inner products of length m one term after the other, so at
# m = 262145 their rounding error is of random-walk size sqrt(m) eps = 512 eps (Higham, Accuracy and Stability of Numerical
# Algorithms, 2nd ed., section 4.2; worst case m eps), beside which the l + 4 = 21 of the R bar does not count.  It measures
# 2.58 of the bar there.  For this library and this case alone the constant is l + 4 + sqrt(m); LAPACK (0.042 of the bar:
# blocked sums), the restatement and the HIP kernels keep the bar as stated.
WIDEN = {("cpu_library", "262145x17"): {"R": (17 + 4 + np.sqrt(262145.0)) / (17 + 4)}}


def lapack_qr(Y):
    return np.linalg.qr(Y, mode="reduced")


@pytest.fixture(scope="module")
def cpu_qr(gsi):
    c = gsi.Context(0, lib=cpuref.load_cpuref())
    yield lambda Y: gsi.qr_thinQ(Y, return_R=True, ctx=c)
    c.close()
    for who in sorted(hc.MEASURED):
        worst = {}
        for name, ratios in hc.MEASURED[who].items():
            for bar, v in ratios.items():
                if v >= worst.get(bar, (-1.0, ""))[0]:
                    worst[bar] = (v, name)
        print(who, "largest ratio per bar:", {k: ("%.3g" % v, n) for k, (v, n) in worst.items()})


@pytest.fixture(params=["lapack", "cpu_library"])
def backend(request, cpu_qr):
    return request.param, (lapack_qr if request.param == "lapack" else cpu_qr)


@pytest.mark.parametrize("case", ALL_FULL, ids=lambda c: c.name)
def test_table(backend, case):
    who, qr = backend
    hc.check_case(qr, case, who=who, widen=WIDEN.get((who, case.name)))


def test_reference_conditioning():
    """Every full-rank case but the one without a reference has kappa_2(Y_n) < 1e3, so its R and Q are pinned."""
    for case in hc.FORCED + hc.GATE:
        if case.name not in hc.NO_REFERENCE:
            assert hc.reference(case)["kappa"] < 1e3, case.name
    assert hc.reference(hc.SCALE_BASE)["kappa"] < 1e3


@pytest.mark.parametrize("name", hc.EXACT)
def test_exact(backend, name):
    hc.check_exact(backend[1], name)


def test_scaling_cpu_library(cpu_qr):
    """The CPU library returns the same bits at every scale (its norms are scaled)."""
    Y = hc.reference(hc.SCALE_BASE)["Y"]
    base = cpu_qr(Y.copy(order="F"))
    for s in hc.SCALINGS + hc.RANGES:
        hc.check_scaling(cpu_qr, s, base=base)


@pytest.mark.parametrize("s", hc.RANGES)
def test_range(gsi, backend, s):
    who, qr = backend
    assert hc.check_range(qr, s, (gsi.GsiError,), who=who) is not None
