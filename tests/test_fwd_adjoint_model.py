"""CPU checks of the adjoint of a sparse forward model, no GPU and no library:
1. The numpy model (tests/fwd_adjoint_model.py): its plan on the crafted inputs, and its sum in plan order against longdouble
   within (k_j + 4) 2^-53 sum_t |h_t| |V| -- k_j - 1 additions, one product, the one rounding of vals * w, then slack.
2. The C++ planner and host sum (csrc/fwd_adjoint_plan.hpp, csrc/fwd_adjoint_host.hpp) built stand-alone with the address and
   undefined-behaviour sanitizers (tests/fwd_adjoint_check.cpp): its own brute-force checks, and the index compared with the
   model entry for entry."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fwd_adjoint_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = fm.CHUNK


# ---- 1. the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 257, 1000])
def test_fan_has_the_lists_it_promises(n):
    indptr, indices, data, lengths = fm.fan(n)
    pl = fm.plan(indptr, indices, data, n)
    assert len(indptr) - 1 == 3 * CHUNK + 5
    lens = np.diff(pl["colptr"])
    assert np.array_equal(lens, lengths)
    assert set(fm.FAN_LENGTHS) <= set(lens.tolist()) and lens[0] in fm.FAN_LENGTHS and lens[-1] in fm.FAN_LENGTHS
    rows = np.diff(indptr)
    assert (rows == 0).sum() >= 2                                               # empty rows
    unsorted = repeated = False
    for r in range(len(rows)):
        j = indices[indptr[r]:indptr[r + 1]]
        unsorted |= bool((np.diff(j) < 0).any())
        repeated |= len(set(j.tolist())) < len(j)
    assert unsorted and repeated
    # the long columns and their chunks
    assert np.array_equal(pl["long_col"], np.flatnonzero(lens > CHUNK))
    assert len(pl["chunk_off"]) == int(np.ceil(lens[lens > CHUNK] / CHUNK).sum()) and pl["maxlen"] == 3 * CHUNK + 5
    for j in range(n):                                                          # lists by ascending row
        assert (np.diff(pl["row"][pl["colptr"][j]:pl["colptr"][j + 1]]) >= 0).all()


@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("n", [256, 1000])
def test_model_sum_against_longdouble(n, with_w):
    indptr, indices, data, lengths = fm.fan(n)
    w = fm.weights(n) if with_w else None
    pl = fm.plan(indptr, indices, data, n, w)
    V = np.random.default_rng(n).standard_normal((len(indptr) - 1, 3))
    G = fm.adjoint(pl, V)
    # the reference: exact products of the unrounded factors, in longdouble
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    Hl = np.zeros((len(indptr) - 1, n), dtype=fm.LD)
    wl = np.ones(n, dtype=fm.LD) if w is None else w.astype(fm.LD)
    np.add.at(Hl, (rows, indices), data.astype(fm.LD) * wl[indices])
    ref = Hl.T @ V.astype(fm.LD)
    scale = fm.adjoint_abs(pl, V)
    bound = (lengths[:, None] + 4) * fm.EPS * scale
    err = np.abs(G.astype(fm.LD) - ref)
    assert (G[lengths == 0] == 0.0).all() and not np.signbit(G[lengths == 0]).any()
    ratio = float((err[scale > 0] / bound[scale > 0]).max())
    print(f"n={n} w={with_w}: max err / bound = {ratio:.3f}")
    assert (err <= bound).all(), ratio
    # the model's own longdouble sum differs from that reference by the rounding of vals * w alone
    assert (np.abs(fm.adjoint_ld(pl, V) - ref) <= (1 if with_w else 0) * fm.EPS * scale + 64 * 2.0 ** -63 * scale).all()


def test_model_on_integers_is_exact():
    n = 257
    indptr, indices, data, _ = fm.fan(n, values="int")
    pl = fm.plan(indptr, indices, data, n)
    V = np.random.default_rng(2).integers(-8, 9, size=(len(indptr) - 1, 2)).astype(float)
    assert np.array_equal(fm.adjoint(pl, V), fm.dense(indptr, indices, data, n).T @ V)


# ---- 2. the planner under sanitizers -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the planner check"
    exe = str(tmp_path_factory.mktemp("fwd_adjoint") / "fwd_adjoint_check")
    src = os.path.join(ROOT, "tests", "fwd_adjoint_check.cpp")
    inc = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True)
    return exe


def test_planner_and_host_sum_under_sanitizers(planner):
    r = subprocess.run([planner, "--chunk"], capture_output=True, text=True, check=True)
    assert int(r.stdout) == CHUNK
    r = subprocess.run([planner, "--self"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("checked"), r.stdout + r.stderr


@pytest.mark.parametrize("chunk", [1, 3, None])
@pytest.mark.parametrize("with_w", [False, True])
def test_planner_equals_the_model(planner, tmp_path, with_w, chunk):
    n = 257
    indptr, indices, data, _ = fm.fan(n)
    w = fm.weights(n) if with_w else None
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "index.bin")
    with open(case, "wb") as f:
        np.array([len(indptr) - 1, n, len(indices), int(with_w)], dtype=np.int64).tofile(f)
        indptr.tofile(f)
        indices.tofile(f)
        data.tofile(f)
        if with_w:
            w.tofile(f)
    r = subprocess.run([planner, case, out] + ([str(chunk)] if chunk else []), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("indexed"), r.stdout + r.stderr
    pl = fm.plan(indptr, indices, data, n, w, chunk or CHUNK)
    raw = np.fromfile(out, dtype=np.int64)
    nlong, nchunk, maxlen = (int(v) for v in raw[:3])
    assert (nlong, nchunk, maxlen) == (len(pl["long_col"]), len(pl["chunk_off"]), pl["maxlen"])
    at, nnz = 3, pl["nnz"]
    for name, count, as_double in (("colptr", n + 1, False), ("row", nnz, False), ("val", nnz, True), ("long_col", nlong, False),
                                   ("long_chunk0", nlong + 1, False), ("chunk_off", nchunk, False), ("chunk_len", nchunk, False)):
        got = raw[at:at + count]
        at += count
        want = pl[name]
        assert np.array_equal(got.view(np.float64) if as_double else got, want.astype(np.float64 if as_double else np.int64)), name
    assert at == raw.size
