"""CPU checks behind tests/test_jacobi_svd_gpu.py: the model of the block Jacobi SVD (tests/jacobi_svd_model.py), the
dispatch table of the GPU cases, the bound the GPU cases assert, and the schedule builder as a host program.

  * every column pair is visited exactly once per inner sweep by the kernel's order, for 16, 8, 4 and 2 columns per block
    and ragged widths (counted);
  * dispatch() agrees with what each GPU case says it reaches, and every case fits the LDS request;
  * the float64 model of the scheme sits at <= 0.25 of the bound l eps kappa_2(W_n) on every graded GPU input (so the bound
    is never one a correct float64 implementation misses), scaled inputs and forced widths included;
  * deliberately wrong variants of the model (a block of columns never rotated, no tie rule) miss the bars of the GPU
    cases -- those bars can tell;
  * csrc/jacobi_sched.hpp (tournament and sparse schedule), compiled with the address and undefined-behaviour sanitizers
    into a program of its own (tests/host/jacobi_sched_main.cpp) and run.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jacobi_svd_model as jm
import test_jacobi_svd_gpu as tg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL_SHARE = 0.25                     # of the bound: what the float64 model may use


# ---- the order of pairs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [16, 8, 4, 2])
@pytest.mark.parametrize("l", [1, 2, 3, 15, 16, 17, 31, 32, 33, 40, 41, 48, 63, 65, 96, 97])
def test_every_column_pair_once_per_sweep(l, w):
    V = jm.visit_counts(l, w)                                  # also asserts that every step's pairs are disjoint
    assert np.array_equal(V, 1 - np.eye(l, dtype=np.int64)), (l, w)


def test_rr_pair_is_a_tournament():
    for n in (2, 4, 6, 32, 38):
        met = set()
        for r in range(n - 1):
            rnd = [jm.rr_pair(n, r, q) for q in range(n // 2)]
            assert len({x for p in rnd for x in p}) == n
            met |= {(min(p), max(p)) for p in rnd}
        assert len(met) == n * (n - 1) // 2


# ---- dispatch ----------------------------------------------------------------------------------------------------------------
def test_dispatch_agrees_with_the_gpu_case_tables():
    for n, l, expect in tg.GRADED_CHOLQR + tg.GRADED_HOUSEHOLDER + tg.LIMITS:
        d = jm.dispatch(l)
        for k, v in expect.items():
            assert d[k] == v, ((n, l), k, d[k], v)
        assert d["lds_bytes"] <= jm.LDS_REQUEST, (l, d)
    for n, l, _ in tg.GRADED_CHOLQR:
        assert n >= 2 * l and l <= 1024
    for n, l, _ in tg.GRADED_HOUSEHOLDER:
        assert n < 2 * l
    for w in tg.FORCED_WIDTHS:
        for l in tg.FORCED_L:
            d = jm.dispatch(l, w)
            assert d["svd_w"] == w and not d["activity"] and d["lds_bytes"] <= jm.LDS_REQUEST
    for l, blocks, _ in tg.SPARSE:
        d = jm.dispatch(l)
        assert d["activity"] and d["first_look"] == 1 and max(blocks) < d["nblk"]


def test_dispatch_thresholds():
    got = {l: jm.dispatch(l)["svd_w"] for l in (1, 600, 601, 1200, 1201, 2500, 2501, 5000)}
    assert got == {1: 16, 600: 16, 601: 8, 1200: 8, 1201: 4, 2500: 4, 2501: 2, 5000: 2}
    assert jm.dispatch(700, 16)["svd_w"] == 8 and jm.dispatch(1300, 8)["svd_w"] == 4 and jm.dispatch(2600, 4)["svd_w"] == 2
    assert jm.dispatch(96, 2)["svd_w"] == 2
    # the widths at the LDS limit of each blocking (a 163,776 B request) and the first one past it
    assert [jm.dispatch(l)["lds_bytes"] for l in (600, 1200, 2500)] == [159760, 153616, 160784]
    assert jm.dispatch(5000)["lds_bytes"] <= jm.LDS_REQUEST
    assert jm.dispatch(32)["nblk"] == 2 and jm.dispatch(33)["nblk"] == 4 and jm.dispatch(33)["lp"] == 48


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def test_graded_inputs_are_what_the_docstrings_say():
    B = jm.hashed_ints(70, 33)
    assert B.min() == -8 and B.max() == 8 and np.array_equal(B, np.round(B))
    assert not np.array_equal(B, jm.hashed_ints(70, 33, seed=1))
    W = jm.graded(70, 33)
    m, e = np.frexp(W[W != 0])
    assert np.array_equal(m * 32, np.round(m * 32)) and e.min() >= -40 and e.max() <= 4      # dyadic, 2^-40 .. 8
    for (n, l), lo, hi in [((70, 33), 4.5, 5.4), ((330, 160), 4.5, 5.4), ((50, 33), 6.0, 16.0), ((130, 96), 9.0, 16.0)]:
        assert lo <= jm.kappa_normalised(jm.graded(n, l)) <= hi, (n, l)
    with np.load(tg.GOLDEN) as g:
        for n, l in [(520, 256), (650, 320), (1210, 601)]:
            assert jm.exact_sum(jm.graded(n, l)) == float(g[f"sum_{n}_{l}"])
            assert g[f"S_{n}_{l}"].shape == (l,) and np.all(np.diff(g[f"S_{n}_{l}"]) < 0)


def test_svd_ref_against_closed_forms():
    d = np.ldexp(1.0, -np.arange(0, 60, 3))
    Q, _ = np.linalg.qr(jm.hashed_ints(40, 20, seed=9))
    assert np.allclose(np.asarray(jm.svd_ref(Q * d), dtype=np.float64), d, rtol=1e-14, atol=0)     # orthogonal columns, graded
    W = jm.hashed_ints(30, 12, seed=2)
    s = np.asarray(jm.svd_ref(W), dtype=np.float64)
    assert np.allclose(s, np.linalg.svd(W, compute_uv=False), rtol=1e-13, atol=0)
    assert abs(float((jm.svd_ref(W) ** 2).sum()) - float((W * W).sum())) < 1e-12            # ||W||_F^2, an exact integer


# ---- the model against the reference: the share of the bound ----------------------------------------------------------------
def model_ratio(n, l, w, scale=1.0, **wrong):
    W, ref, bound = tg.graded_case(n, l)
    S, U, info = jm.svd_model(jm.device_R(W * scale), w, **wrong)
    assert wrong or info["converged"]
    with np.errstate(invalid="ignore"):
        rel = np.abs(S.astype(np.longdouble) - ref * np.longdouble(scale)) / (ref * np.longdouble(scale))
    return float(np.nan_to_num(np.asarray(rel, dtype=np.float64), nan=np.inf).max()) / bound


@pytest.mark.parametrize("n,l", [(n, l) for n, l, _ in tg.GRADED_CHOLQR + tg.GRADED_HOUSEHOLDER])
def test_model_within_a_quarter_of_the_bound(n, l):
    ratio = model_ratio(n, l, jm.dispatch(l)["svd_w"])
    print(f"({n}, {l}): model / bound = {ratio:.3f}")
    assert ratio <= MODEL_SHARE


@pytest.mark.parametrize("n,l", tg.SCALED)
@pytest.mark.parametrize("bits", [120, -120])
def test_model_scaled_within_a_quarter_of_the_bound(n, l, bits):
    assert model_ratio(n, l, 16, scale=float(np.ldexp(1.0, bits))) <= MODEL_SHARE


@pytest.mark.parametrize("w", [16, 8, 4, 2])
def test_model_all_widths_within_a_quarter_of_the_bound(w):
    for l in tg.FORCED_L:
        ratio = model_ratio(2 * l + 4, l, w)
        assert ratio <= MODEL_SHARE, (l, w, ratio)


# ---- wrong variants must miss the GPU cases' bars ----------------------------------------------------------------------------
WRONG_GRADED = [(n, l) for n, l, _ in tg.GRADED_CHOLQR + tg.GRADED_HOUSEHOLDER if 2 <= l <= 176]


@pytest.mark.parametrize("n,l", WRONG_GRADED)
def test_a_skipped_block_misses_the_relative_bound(n, l):
    """The last block of columns never rotated (a wrong loop bound, a padding block mishandled): every graded case from two
    columns on leaves the bound far behind.  (A rotation threshold 1000 times too large does NOT show in the singular values
    of these inputs: Jacobi converges quadratically, the sweep that brings every pair below 1000 tol brings most far below
    tol, and what is left moves a singular value in second order.  The model with tol_scale=1e3 stays inside the same
    quarter of the bound; that mistake costs orthogonality of the vectors, not S.)"""
    assert model_ratio(n, l, jm.dispatch(l)["svd_w"], skip_block=-1) > 1.0


def test_wrong_variants_miss_the_exact_cases():
    W, d = tg.diagonal_input(33)
    order = np.argsort(-d, kind="stable")
    S, U, _ = jm.svd_model(jm.cholqr2_R(W), 16)
    assert np.array_equal(S, d[order]) and np.array_equal(U[order, np.arange(33)], np.ones(33))
    S, U, _ = jm.svd_model(jm.cholqr2_R(W), 16, tie_rule=False)       # equal norms ranked equally: slots nobody writes
    assert not np.array_equal(S, d[order])


# ---- the sparse-schedule inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,blocks", [(l, b) for l, b, _ in tg.SPARSE])
def test_sparse_inputs_stay_active_for_three_sweeps(l, blocks):
    """After the first sweep only pairs inside the dense set couple, and the model is still active (4 tol) after its second
    sweep: the device needs a third, and sweeps two and three run on a schedule."""
    W = tg.sparse_input(l, blocks)
    R = jm.device_R(W)
    inset = np.zeros(l, dtype=bool)
    for b in blocks:
        inset[16 * b:16 * b + 16] = True
    G = R.T @ R
    off = G - np.diag(np.diag(G))
    assert np.abs(off[~inset]).max() == 0.0                     # columns outside the set: exactly orthogonal to everything
    S, U, info = jm.svd_model(R, 16)
    assert info["converged"] and info["active_after"][0] and info["active_after"][1], info
    assert np.abs(S - np.linalg.svd(W, compute_uv=False)).max() <= 1e-12 * S[0]


# ---- the schedule builder as a host program ----------------------------------------------------------------------------------
def test_schedule_builder_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "jacobi_sched_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-Wall", "-I", os.path.join(ROOT, "geostatinversion.jl_amd", "csrc"),
                        os.path.join(HERE, "host", "jacobi_sched_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "jacobi-sched-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
