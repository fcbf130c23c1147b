"""The case table of test_fft_pass_kernels_gpu.py reaches what it claims to reach, by the launcher model of
fft_pass_model.py; its exact reference is right; and the bar it sets is attainable.  No GPU.

The conditions (a) .. (j) are statements about the table, not measurements: a table that misses one fails here."""
import json
import os

import numpy as np
import pytest

import fft_pass_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12

LAUNCHES = [(case, p) for case in fm.CASES for p in fm.passes(*case)]


def dims(case):
    return len(case[0])


def where(**kw):
    """The launches whose fields equal the keywords (a callable value is a predicate on the field)."""
    out = []
    for case, p in LAUNCHES:
        if all(v(p[k]) if callable(v) else p[k] == v for k, v in kw.items()):
            out.append((case, p))
    return out


def pow2s(lo, hi):
    return {1 << e for e in range(fm.ilog2(lo), fm.ilog2(hi) + 1)}


def test_table_limits():
    assert len(set(fm.CASES)) == len(fm.CASES)
    for Ns, l in fm.CASES:
        n = int(np.prod(Ns))
        assert n <= 4 * 10 ** 4 and n * l <= 2 * 10 ** 6 and min(Ns) >= 2 and max(Ns) <= 4096, (Ns, l)
    for case in fm.CASES_1D + fm.CASES_2D_NATURAL + fm.CASES_3D_NATURAL:
        assert all(p["lb"] == 0 for p in fm.passes(*case)), case
    for case in fm.BLOCKED_CASES:
        assert all(p["lb"] == 4 for p in fm.passes(*case)), case


def test_a_every_reachable_instantiation():
    """Ma = 2 cannot occur: an axis of one point is squeezed away, and N >= 2 embeds to M >= 4 -- so <*, 1, true> is dead."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "isa_resources.json")))["kernels"]
    names = {k for k in rec if k.startswith("gsi::hipk::fft_pass_kernel<")}
    assert len(names) == 42
    dead = {fm.inst_name((m, 1, True)) for m in fm.MODES}
    assert dead <= names
    reached = {fm.inst_name(p["inst"]) for _, p in LAUNCHES}
    assert reached == names - dead and len(reached) == 36
    assert all(fm.embed(N) >= 4 for N in range(2, 4097))


def test_b_every_line_length():
    assert {p["Ma"] for _, p in where(mode=15)} == pow2s(4, 8192)
    assert {p["Ma"] for _, p in where(mode=3)} == pow2s(4, 8192)
    assert {p["Ma"] for _, p in where(mode=25)} == pow2s(4, 8192)
    assert {p["Ma"] for _, p in where(mode=4)} == pow2s(4, 8192)
    assert {p["Ma"] for _, p in where(mode=0)} == pow2s(4, 4096)
    assert {p["Ma"] for _, p in where(mode=16)} == pow2s(4, 4096)
    for mode in (15, 3, 25):
        assert {p["wpl"] for _, p in where(mode=mode)} == {1, 2, 4, 8}
    assert {p["T"] for _, p in where(mode=4)} == {1, 2, 4, 8, 16}
    for mode in (0, 16):                                  # Ma <= 4096 there: T >= 2
        assert {p["T"] for _, p in where(mode=mode)} == {2, 4, 8, 16}
        assert {p["wpl"] for _, p in where(mode=mode)} == {1, 2, 4}
    assert {p["wpl"] for _, p in where(mode=4)} == {1, 2, 4, 8}


def test_c_both_branches_of_s_lin():
    for mode in (0, 4, 16):
        assert {p["s_lin"] for _, p in where(mode=mode)} == {True, False}, mode


def test_d_both_layouts():
    """MODE 15 is the 1-D pass, and the blocked layout needs a strided pass (d >= 2): it is natural only."""
    assert {p["lb"] for _, p in where(mode=15)} == {0}
    for mode in (3, 25, 4, 0, 16):
        assert {p["lb"] > 0 for _, p in where(mode=mode)} == {False, True}, mode
    k1_2d = [p for c, p in where(mode=4, kind=1) if dims(c) == 2]
    assert k1_2d and all(p["OS"] == 0 for p in k1_2d)
    for mode in (0, 16):
        k1 = [p for c, p in where(mode=mode, kind=1) if dims(c) == 3]
        assert k1 and all(p["OS"] == 16 for p in k1), mode
    assert [p for c, p in where(mode=4, kind=2) if dims(c) == 3]
    # both layouts of the axis-0 passes in 2-D and in 3-D (S1 / S2 of off() differ between them)
    for mode in (3, 25):
        for d in (2, 3):
            assert {p["lb"] > 0 for c, p in where(mode=mode) if dims(c) == d} == {False, True}, (mode, d)


def test_e_ragged_and_full_last_tiles():
    for mode in (3, 25):
        assert {p["ragged"] for _, p in where(mode=mode)} == {True, False}, mode


def test_f_both_forms_of_off():
    for mode in (3, 25):
        assert {p["off_form"] for _, p in where(mode=mode)} == {"uniform", "division"}, mode
    for lb in (0, 4):
        assert {p["off_form"] for _, p in where(mode=3, lb=lb)} == {"uniform", "division"}, lb


def test_g_looping_launches():
    assert not where(mode=15, looping=True)
    assert all(p["nitems"] <= 64 for _, p in where(mode=15))          # one line per pair, at most 64 pairs a batch
    for mode in (3, 25, 4, 0, 16):
        assert where(mode=mode, looping=True, nb=lambda nb: nb >= 2), mode
    assert where(mode=4, looping=True, threads=512, nb=lambda nb: nb >= 2)
    assert where(mode=0, looping=True, threads=512, nb=lambda nb: nb >= 2) or \
        where(mode=16, looping=True, threads=512, nb=lambda nb: nb >= 2)
    assert where(mode=3, looping=True, ragged=True) and where(mode=25, looping=True, ragged=True)


def test_h_both_item_orders():
    for mode in fm.MODES:
        g = {p["G"] % 8 == 0 for _, p in where(mode=mode, looping=False, G=lambda G: G is not None)}
        assert g == {True, False}, mode


def test_i_second_pair_batch():
    odd = False
    for d in (1, 2, 3):
        hit = [(c, p) for c, p in where(col0=lambda c0: c0 > 0) if dims(c) == d]
        assert hit, d
        odd = odd or any(c[1] % 2 == 1 for c, _ in hit)
    assert odd


def test_j_column_counts():
    for d in (1, 2, 3):
        ls = {l for Ns, l in fm.CASES if len(Ns) == d}
        assert 1 in ls and any(l % 2 == 0 for l in ls) and any(l % 2 == 1 and l > 1 for l in ls), d


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in fm.CASES if np.prod(c[0]) <= 2000], ids=fm.case_id)
def test_structured_reference_is_the_dense_index_product(case):
    Ns, l = case
    tab, X = fm.int_table(Ns), fm.int_panel(Ns, min(l, 5))
    assert np.array_equal(fm.structured_reference(tab, X), fm.dense_reference(tab, X))


def test_inputs_are_integers_without_extra_symmetry():
    tab, X = fm.int_table((17, 17)), fm.int_panel((17, 17), 4)
    assert np.array_equal(tab, np.round(tab)) and np.abs(tab).max() <= 3
    assert np.array_equal(X, np.round(X)) and np.abs(X).max() <= 4
    assert not np.array_equal(tab, tab.T)                 # a square grid's table is not invariant under swapping its axes


@pytest.mark.parametrize("case", [c for c in fm.CASES if np.prod(c[0]) <= 4096], ids=fm.case_id)
def test_host_fft_meets_the_bar(case):
    """numpy's double-precision FFT of the same embedding against the exact product: the 1e-12 bar of the GPU test is
    attainable for these inputs (observed: at most 3.8e-16)."""
    Ns, l = case
    tab, X = fm.int_table(Ns), fm.int_panel(Ns, l)
    Yref = fm.exact_reference(tab, X)
    scale = np.abs(Yref).max()
    assert scale > 0
    ratio = np.abs(fm.host_fft_product(tab, X) - Yref).max() / scale
    print(f"{fm.case_id(case)} host FFT {ratio:.2e}")
    assert ratio <= BAR
