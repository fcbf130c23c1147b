"""The sample-space tail of a LowRankCovMatrix randsvd with its side product forked at B0.

Z = S B1 M and B1 = B0 XW1, so Z[0:n_f] = (S[0:n_f] B0) (XW1 M): Backend::lowrank_tail forms Y_f = S[0:n_f] B0 on its second
stream as soon as B0 = c G A1 exists (behind the first product of the second Gram round) instead of waiting for B1 (behind
the fourth round), and multiplies by N' = XW1 M at the end.  GSI_LOWRANK_TAIL_FORK=late keeps the fork behind the fourth round.
What must hold between the three legs -- forked early, forked late, overlap off (GSI_LOWRANK_TAIL_OVERLAP=0):

  * the singular values bit for bit (their chain is the same launches on the same data), and the rows of Z from n_f on bit
    for bit (the row block of the same product on the same C);
  * the rows before n_f within 1e-12 sqrt(sigma_1) on the columns' distance, the bar of tests/test_lowrank_tail_gpu.py;
  * the last l - K columns exactly zero (they are cleared on the second stream now), one overlap counted per call, a second
    call bit for bit the first, device memory back to what it was;
  * gsi_ctx_path_info's LOWRANK_TAIL_SERIES_ROUNDS: the same count in every leg and call, at least the last round of each
    tail, none under GSI_CQ_SERIES=0, whose sigma agree within 1e-13 relative and whose Z Z' within 2e-12 sigma_1;
  * a tail that declines (decay 2.5: the check of a refinement round fails, with the side product already in flight when
    forked early) leaves the bits and counters of the leg without the overlap, and counts no overlap.

n = 3000, N_s = 400; forced row fractions 0.05 (n_f = 128, one tile) and 0.94 (n_f = 2816: one full tile and a ragged one in
the direct part); l = 48, 160, 320, q = 0 and 1, K < l and K = l.  The switches are read once per process: each leg is one
child process that runs every shape, the six side by side (the sixth: GSI_CQ_SERIES=0, the refinement rounds by Cholesky).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3000
NS = 400

CHILD = r'''
import json, sys, numpy as np
import gsi_amd as gsi
out, cases = sys.argv[1], json.loads(sys.argv[2])
res = {}
for name, (n, Ns, K, p, q, decay) in cases.items():
    ctx = gsi.Context(0)                 # one per shape: counters and the QR tier hints start from nothing in every leg
    def fresh():
        op = gsi.lowrank_synthetic_operator(ctx, n, Ns, seed=0, decay=decay)
        Om = gsi.DeviceMatrix(ctx, n, K + p).randn(7)
        Z = gsi.DeviceMatrix(ctx, n, K + p).randn(11)      # (not zero: the last columns must be cleared, not found clear)
        return op, Om, Z, gsi.DeviceMatrix(ctx, K + p, 1)
    def run(op, Om, Z, S):
        gsi._lib.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, S.h), ctx.lib)
        return Z.to_host(), S.to_host()[:, 0]
    hs = fresh()
    pi0 = ctx.path_info()
    Z1, S1 = run(*hs)
    pi1 = ctx.path_info()
    Z2, S2 = run(*hs)
    pi2 = ctx.path_info()
    counters = ctx.counters()
    for h in hs:
        h.close()
    ctx.release_cache()
    before = ctx.device_bytes()          # every workspace of this shape exists by now
    hs = fresh()
    run(*hs)
    for h in hs:
        h.close()
    ctx.release_cache()
    np.save(out + "_" + name + "_S.npy", S1)
    np.save(out + "_" + name + "_Z.npy", Z1)
    res[name] = {"overlaps": [pi1["lowrank_tail_overlaps"] - pi0["lowrank_tail_overlaps"], pi2["lowrank_tail_overlaps"] - pi1["lowrank_tail_overlaps"]],
                 "tails": [pi1["lowrank_tails"] - pi0["lowrank_tails"], pi2["lowrank_tails"] - pi1["lowrank_tails"]],
                 "series": [pi1["lowrank_tail_series_rounds"] - pi0["lowrank_tail_series_rounds"],
                            pi2["lowrank_tail_series_rounds"] - pi1["lowrank_tail_series_rounds"]],
                 "repeat_identical": bool(np.array_equal(Z1, Z2, equal_nan=True) and np.array_equal(S1, S2, equal_nan=True)),
                 "zero_tail": bool(np.all(Z1[:, K:] == 0.0)), "counters": counters,
                 "bytes_before": before, "bytes_after": ctx.device_bytes()}
    ctx.close()
print("result " + json.dumps(res))
'''

# name: (n, N_s, K, p, q, decay)
SHAPES = {
    "l48_q1": (N, NS, 32, 16, 1, 0.75),
    "l48_q0": (N, NS, 32, 16, 0, 0.75),
    "l160_q1_full": (N, NS, 160, 0, 1, 0.75),
    "l160_q0": (N, NS, 128, 32, 0, 0.75),
    "l320_q1": (N, NS, 256, 64, 1, 0.75),
    "l320_q0_full": (N, NS, 320, 0, 0, 0.75),
    "decline": (N, NS, 32, 16, 1, 2.5),
}
RUN = [k for k in SHAPES if k != "decline"]
# leg: (GSI_LOWRANK_TAIL_OVERLAP, GSI_LOWRANK_TAIL_FORK or None, GSI_CQ_SERIES or None)
LEGS = {
    "off": ("0", None, None),
    "early_one_tile": ("0.05", None, None),
    "early_ragged": ("0.94", None, None),
    "late_one_tile": ("0.05", "late", None),
    "late_ragged": ("0.94", "late", None),
    "early_ragged_cholesky": ("0.94", None, "0"),
}
NF = {"one_tile": 128, "ragged": 2816}


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tail_fork")
    procs = {}
    for leg, (overlap, fork, series) in LEGS.items():
        env = dict(os.environ)
        for k in ("GSI_LOWRANK_TAIL_OVERLAP", "GSI_LOWRANK_TAIL_RESERVE_CUS", "GSI_LOWRANK_TAIL_FORK", "GSI_NO_LOWRANK_TAIL",
                  "GSI_NO_LOWRANK_POWER", "GSI_NO_LOWRANK_SPLIT", "GSI_NO_CHOLQR", "GSI_CQ_SERIES"):
            env.pop(k, None)
        env["GSI_LOWRANK_TAIL_OVERLAP"] = overlap
        if fork is not None:
            env["GSI_LOWRANK_TAIL_FORK"] = fork
        if series is not None:
            env["GSI_CQ_SERIES"] = series
        procs[leg] = subprocess.Popen([sys.executable, "-c", CHILD, str(tmp / leg), json.dumps(SHAPES)],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT)
    out = {}
    for leg, pr in procs.items():
        so, se = pr.communicate(timeout=600)
        assert pr.returncode == 0, (leg, so[-2000:] + se[-4000:])
        res = json.loads([s for s in so.splitlines() if s.startswith("result ")][-1][len("result "):])
        for name, r in res.items():
            r["S"] = np.load(str(tmp / leg) + "_" + name + "_S.npy")
            r["Z"] = np.load(str(tmp / leg) + "_" + name + "_Z.npy")
        out[leg] = res
    return out


def _small(r):
    return {k: v for k, v in r.items() if k not in ("S", "Z")}


def _check(new, old, old_overlaps, nf, name, what):
    n, Ns, K, p, q, decay = SHAPES[name]
    assert old["overlaps"] == [old_overlaps] * 2 and old["tails"] == [1, 1], _small(old)
    assert new["tails"] == [1, 1] and new["overlaps"] == [1, 1], _small(new)
    for r in (new, old):
        assert r["repeat_identical"] and r["zero_tail"], _small(r)
        assert r["bytes_after"] == r["bytes_before"], _small(r)
    assert new["counters"] == old["counters"], (new["counters"], old["counters"])
    # the refinement rounds see the same Gram matrices in every leg: as many of the two go by series, on every call
    assert new["series"] == old["series"] and new["series"][0] == new["series"][1] and 0 <= new["series"][0] <= 2, \
        (_small(new), _small(old))
    assert np.array_equal(new["S"], old["S"])
    assert np.array_equal(new["Z"][nf:], old["Z"][nf:])
    d = new["Z"][:nf, :K] - old["Z"][:nf, :K]
    err = float(np.max(np.linalg.norm(d, axis=0)))
    bar = 1e-12 * np.sqrt(old["S"][0])
    print(f"\n{name}, {what}: n_f = {nf}, l = {K + p}, K = {K}, q = {q}: max column distance over rows < n_f {err:.3e} "
          f"(bar {bar:.3e}), rows that differ at all: {int(np.count_nonzero(np.any(d != 0.0, axis=1)))}")
    assert err <= bar, (err, bar)
    assert np.all(new["Z"][:, K:] == 0.0)


@pytest.mark.parametrize("name", RUN)
@pytest.mark.parametrize("frac", ["one_tile", "ragged"])
def test_early_fork_against_late_and_off(legs, frac, name):
    early = legs["early_" + frac][name]
    _check(early, legs["late_" + frac][name], 1, NF[frac], name, "early against late")
    _check(early, legs["off"][name], 0, NF[frac], name, "early against overlap off")


def test_series_rounds_are_taken_in_the_tail_and_counted(legs):
    """Inside lowrank_tail (tmp in a buffer of the chain, the skip word and the count in the backend's flag words, read with the
    verdict): the count rises by the rounds that went by series, and stays 0 under GSI_CQ_SERIES=0, where the tail must still
    agree with the series leg: sigma within 1e-13 relative, Z Z' to the equivalent of the column bar (R and R^-1 differ in
    rounding only)."""
    taken = {name: legs["early_ragged"][name]["series"] for name in RUN}
    print("\nseries rounds per call:", taken)
    # the last refinement round factors the Gram matrix of a panel that is orthonormal to rounding (|E|_F ~ l eps << 6e-6)
    assert all(t[0] >= 1 for t in taken.values()), taken
    for name in RUN:
        on, off = legs["early_ragged"][name], legs["early_ragged_cholesky"][name]
        n, Ns, K, p, q, decay = SHAPES[name]
        assert off["series"] == [0, 0] and off["tails"] == [1, 1] and off["overlaps"] == [1, 1], _small(off)
        assert off["repeat_identical"] and off["zero_tail"], _small(off)
        rel = float(np.max(np.abs(on["S"] - off["S"]) / off["S"]))
        # Another R in rounding is another input to the small SVD: columns of close singular values may come out rotated among
        # themselves or with the other sign (l320_q0_full: q = 0 and K = l, the last values crowd), so the vectors are compared
        # through Z Z', which no such rotation moves.  Columns within 1e-12 sqrt(sigma_1) of each other, the project's bar, keep
        # |Z Z' - Z0 Z0'|_F within 2 sqrt(sigma_1) * 1e-12 sqrt(sigma_1) * sqrt(K) / sqrt(K) <= 2e-12 sigma_1.
        Zn, Zo = on["Z"][:, :K], off["Z"][:, :K]
        err = float(np.linalg.norm(Zn @ Zn.T - Zo @ Zo.T))
        bar = 2e-12 * off["S"][0]
        print(f"{name}: series {on['series']}, sigma within {rel:.2e} relative, |Z Z' - Z0 Z0'|_F {err:.2e} (bar {bar:.2e})")
        assert rel <= 1e-13 and err <= bar, (name, rel, err, bar)
    assert legs["early_ragged"]["decline"]["series"] == legs["off"]["decline"]["series"]


@pytest.mark.parametrize("leg", ["early_one_tile", "early_ragged", "late_one_tile"])
def test_declined_tail_is_the_ordinary_path(legs, leg):
    new, old = legs[leg]["decline"], legs["off"]["decline"]
    assert new["tails"] == [0, 0] and old["tails"] == [0, 0], (_small(new), _small(old))
    assert new["overlaps"] == [0, 0] and old["overlaps"] == [0, 0], (_small(new), _small(old))
    assert np.array_equal(new["S"], old["S"], equal_nan=True)
    assert np.array_equal(new["Z"], old["Z"], equal_nan=True)
    assert new["counters"] == old["counters"], (new["counters"], old["counters"])
    assert new["repeat_identical"] and new["bytes_after"] == new["bytes_before"], _small(new)
