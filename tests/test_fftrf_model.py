"""The device FFTRF sampler's algorithm and launcher, checked without a GPU (tests/fftrf_model.py).

(a) The numpy model of the device algorithm -- separable inverse DFT with the crop behind every axis, Bluestein where 2 N is
    not a power of two, the axis swap, the two-pass normalisation -- agrees with the oracle's restatement of FFTRF.jl:83-100
    on every case of the table the GPU test walks, fed the same phi, within the bar the GPU test applies to the device.
(b) That table reaches every kernel instantiation the launcher can produce."""
import numpy as np
import pytest

import fftrf_model as fm

ALL = fm.CASES + [fm.BATCH_CASE]


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_model_agrees_with_the_oracle(case):
    worst = 0.0
    for phi in case.phi()[:3]:
        F = fm.field(case.Ns, case.k0, case.dk, case.beta, phi)
        Fref = fm.oracle_field(case.Ns, case.k0, case.dk, case.beta, phi)
        assert F.shape == tuple(case.Ns) and np.isfinite(F).all()
        worst = max(worst, fm.error_ratio(F, Fref, case.k0))
    print(case.id, worst)
    assert worst <= fm.BAR


def test_table_reaches_every_instantiation():
    reached = set()
    for c in ALL:
        reached |= {fm.instantiation(l) for l in fm.launches(c.Ns)}
    want = fm.all_instantiations()
    assert reached <= want, sorted(reached - want)
    assert not want - reached, sorted(want - reached)


def test_table_carries_the_parameter_variants():
    """One case each with beta = +2 and beta = 0, one with k0 != 0 and dk != 1, the rest beta < 0; Bluestein lengths at the
    limits: 3 N - 1 = 2048 exactly, P = 8192, and a direct line of 8192 points."""
    betas = [c.beta for c in fm.CASES]
    assert betas.count(2.0) == 1 and betas.count(0.0) == 1 and all(b < 0 for b in betas if b not in (2.0, 0.0))
    assert any(c.k0 != 0.0 and c.dk != 1.0 for c in fm.CASES)
    lengths = {(l["bluestein"], l["length"]) for c in fm.CASES for l in fm.launches(c.Ns)}
    assert (True, 8192) in lengths and (False, 8192) in lengths and (True, 2048) in lengths
    assert fm.geometry((2, 2, 683))[3][2] == 3 * 683 - 1 == 2048

