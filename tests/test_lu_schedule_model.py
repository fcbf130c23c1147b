"""The block schedule of the single-rank panel LU (csrc/lu_schedule.hpp, through the host-only gsi_lu_schedule): the chooser
returns a minimum of the column-pass model of DESIGN.md 4.2, and GSI_LU_NB / GSI_LU_SCHEDULE give the lists they name.

The model is restated here from the text, not read from the library: with 8-column leaves, a block of s columns costs
4 nl (nl - 1) in-block reads (nl = ceil(s / 8) leaves), the update before a block of s columns at column jb > 0 costs jb + 2 s,
and every block after the first costs BLOCK_PASSES more.  For l <= 256 every valid schedule is enumerated (at most 20 569 of
them); beyond that the enumeration (1.93^(l/16) lists: 7.4 million at l = 384) is replaced by the same exhaustive recursion with
the best continuation from a column remembered -- the cost of a block depends on nothing before it but the column it starts at,
so this is the same minimum."""
import ctypes as C
import functools
import os

import pytest

BLOCK_PASSES = 6     # lu_schedule.hpp: LU_BLOCK_PASSES


def _schedule(gsi, l):
    lib = gsi.load()
    out = (C.c_int32 * ((l + 15) // 16))()
    n = C.c_int32(0)
    st = lib.gsi_lu_schedule(l, out, C.byref(n))
    assert st == 0, lib.gsi_last_error()
    return [int(out[i]) for i in range(n.value)]


def _block(jb, s):
    nl = (s + 7) // 8
    return 4 * nl * (nl - 1) + ((jb + 2 * s + BLOCK_PASSES) if jb > 0 else 0)


def _cost(widths):
    jb = tot = 0
    for s in widths:
        tot += _block(jb, s)
        jb += s
    return tot


def _valid(l, widths):
    return (len(widths) >= 1 and sum(widths) == l and all(1 <= s <= 64 for s in widths)
            and all(s % 16 == 0 for s in widths[:-1]))


def _enumerate(l, jb=0):
    """every valid schedule of the columns [jb, l)"""
    left = l - jb
    if left <= 64:
        yield (left,)
    for s in (16, 32, 48, 64):
        if s < left:
            for rest in _enumerate(l, jb + s):
                yield (s,) + rest


def _best_from(l):
    @functools.lru_cache(maxsize=None)
    def best(jb):
        left = l - jb
        cands = [_block(jb, left)] if left <= 64 else []
        cands += [_block(jb, s) + best(jb + s) for s in (16, 32, 48, 64) if s < left]
        return min(cands)
    return best(0)


@pytest.fixture()
def clean_env(monkeypatch):
    monkeypatch.delenv("GSI_LU_NB", raising=False)
    monkeypatch.delenv("GSI_LU_SCHEDULE", raising=False)
    return monkeypatch


def test_model_restated_here_reproduces_the_documented_pass_counts():
    assert _cost([64, 64, 32]) - 2 * BLOCK_PASSES == 880
    assert _cost([48, 48, 64]) - 2 * BLOCK_PASSES == 832
    assert _cost([32, 32, 48, 48]) - 3 * BLOCK_PASSES == 800
    assert sorted(_enumerate(48)) == [(16, 16, 16), (16, 32), (32, 16), (48,)]


def test_chooser_is_a_minimum_of_the_model(gsi, clean_env):
    for l in range(8, 385):
        w = _schedule(gsi, l)
        assert _valid(l, w), (l, w)
        if l <= 256:
            ref = min(_cost(c) for c in _enumerate(l))
            assert ref == _best_from(l), l
        else:
            ref = _best_from(l)
        assert _cost(w) == ref, (l, w, _cost(w), ref)


def test_ties_go_to_the_first_list_in_dictionary_order(gsi, clean_env):
    for l in (96, 160, 168, 200, 256):
        w = _schedule(gsi, l)
        best = min(_cost(c) for c in _enumerate(l))
        assert tuple(w) == min(c for c in _enumerate(l) if _cost(c) == best), (l, w)


def test_uniform_knob_gives_the_uniform_lists(gsi, clean_env):
    for nb in (32, 64):
        clean_env.setenv("GSI_LU_NB", str(nb))
        for l in (8, 56, 64, 112, 160, 168, 200, 320, 384):
            assert _schedule(gsi, l) == [min(nb, l - jb) for jb in range(0, l, nb)], (nb, l)
    clean_env.setenv("GSI_LU_NB", "64")
    assert _schedule(gsi, 160) == [64, 64, 32]
    assert _schedule(gsi, 200) == [64, 64, 64, 8]
    clean_env.setenv("GSI_LU_NB", "32")
    assert _schedule(gsi, 160) == [32] * 5


def test_forced_list_applies_to_the_width_it_sums_to(gsi, clean_env):
    clean_env.setenv("GSI_LU_SCHEDULE", "16,48,64,32")
    assert _schedule(gsi, 160) == [16, 48, 64, 32]
    clean_env.setenv("GSI_LU_NB", "64")                 # the list wins where it fits, the uniform knob elsewhere
    assert _schedule(gsi, 160) == [16, 48, 64, 32]
    assert _schedule(gsi, 320) == [64] * 5
    clean_env.setenv("GSI_LU_SCHEDULE", "48,48,8")      # a ragged last block
    assert _schedule(gsi, 104) == [48, 48, 8]


@pytest.mark.parametrize("bad", ["48,40,64", "48,,64", "48,80", "abc", "48,48,64,", "0,16", ""])
def test_malformed_list_is_an_error(gsi, clean_env, bad):
    clean_env.setenv("GSI_LU_SCHEDULE", bad)
    lib = gsi.load()
    out = (C.c_int32 * 16)()
    n = C.c_int32(0)
    assert lib.gsi_lu_schedule(160, out, C.byref(n)) == 1       # GSI_ERR_ARG
    assert b"GSI_LU_SCHEDULE" in lib.gsi_last_error()
