"""The sample-space tail of a LowRankCovMatrix randsvd with part of Z formed beside the small SVD.

Backend::lowrank_tail knows B1 (Z = S B1 M) before the chain Cholesky -> Jacobi SVD -> M starts, so it forms Y_f = S[0:n_f] B1
on a second stream while that chain runs, and afterwards Z[0:n_f] = Y_f M (a reduction of length l instead of N_s) and
Z[n_f:n] = S[n_f:n] (B1 M), the row block of the product it ran before.  What must hold against the leg without the overlap
(GSI_LOWRANK_TAIL_OVERLAP=0):

  * the singular values bit for bit (nothing of their chain changed), and the rows of Z from n_f on bit for bit (the same
    tiles of the same product, n_f being a multiple of its 128-row tile);
  * the rows before n_f within the bar tests/test_lowrank_tail_gpu.py applies between its own legs, 1e-12 sqrt(sigma_1) on
    the columns' distance (no sign freedom here: both legs multiply by the same M);
  * one overlap counted per call (gsi_ctx_path_info), a second call bit for bit the first, the last l - K columns zero;
  * device memory back to what it was once operator and matrices are closed (the panel it borrows at q >= 1, the temporary
    it takes at q = 0);
  * a tail that declines leaves the ordinary path's bits and counters, and counts no overlap;
  * without the switch a panel this small is left alone (the default is for panels whose side product runs persistent).

n = 3000, decay 0.75, q = 1, N_s = 200 -- except the l = 320 case: the tail needs l <= N_s - 1 (centred samples span N_s - 1
dimensions; pipeline.cpp: lowrank_tail_applies), so that case has N_s = 400, the smallest round count that lets it run.  The
switches are read once per process: each leg is one child process that runs every shape of that leg, the four side by side.
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
        return op, Om, gsi.DeviceMatrix(ctx, n, K + p), gsi.DeviceMatrix(ctx, K + p, 1)
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
                 "repeat_identical": bool(np.array_equal(Z1, Z2, equal_nan=True) and np.array_equal(S1, S2, equal_nan=True)),
                 "zero_tail": bool(np.all(Z1[:, K:] == 0.0)), "counters": counters,
                 "bytes_before": before, "bytes_after": ctx.device_bytes()}
    ctx.close()
print("result " + json.dumps(res))
'''

# name: (n, N_s, K, p, q, decay)
SHAPES = {
    "l48": (N, 200, 32, 16, 1, 0.75),
    "l320": (N, 400, 256, 64, 1, 0.75),
    "l160": (N, 200, 160, 0, 1, 0.75),
    "q0": (N, 200, 32, 16, 0, 0.75),
    "decline": (N, 200, 32, 16, 1, 2.5),
}
# leg: (GSI_LOWRANK_TAIL_OVERLAP or None, shapes).  0.05 n -> n_f = 128 (one tile); 0.94 n -> n_f = 2816 (n - n_f = 184: one
# full tile and a ragged one in the direct part)
LEGS = {
    "off": ("0", list(SHAPES)),
    "one_tile": ("0.05", ["l48", "q0", "decline"]),
    "ragged": ("0.94", ["l320", "l160"]),
    "default": (None, ["l48"]),
}
NF = {"one_tile": 128, "ragged": 2816}


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tail_overlap")
    procs = {}
    for leg, (value, names) in LEGS.items():
        env = dict(os.environ)
        for k in ("GSI_LOWRANK_TAIL_OVERLAP", "GSI_LOWRANK_TAIL_RESERVE_CUS", "GSI_NO_LOWRANK_TAIL", "GSI_NO_LOWRANK_POWER",
                  "GSI_NO_LOWRANK_SPLIT", "GSI_NO_CHOLQR"):
            env.pop(k, None)
        if value is not None:
            env["GSI_LOWRANK_TAIL_OVERLAP"] = value
        procs[leg] = subprocess.Popen([sys.executable, "-c", CHILD, str(tmp / leg), json.dumps({k: SHAPES[k] for k in names})],
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


def _check_overlapped(legs, leg, name):
    new, old = legs[leg][name], legs["off"][name]
    n, Ns, K, p, q, decay = SHAPES[name]
    nf = NF[leg]
    assert old["overlaps"] == [0, 0] and old["tails"] == [1, 1], _small(old)
    assert new["tails"] == [1, 1] and new["overlaps"] == [1, 1], _small(new)
    for r in (new, old):
        assert r["repeat_identical"] and r["zero_tail"], _small(r)
        assert r["bytes_after"] == r["bytes_before"], _small(r)
    assert new["counters"] == old["counters"], (new["counters"], old["counters"])
    assert np.array_equal(new["S"], old["S"])
    assert np.array_equal(new["Z"][nf:], old["Z"][nf:])
    d = new["Z"][:nf, :K] - old["Z"][:nf, :K]
    err = float(np.max(np.linalg.norm(d, axis=0)))
    bar = 1e-12 * np.sqrt(old["S"][0])
    print(f"\n{name}: n_f = {nf}, l = {K + p}, K = {K}, q = {q}: max column distance over rows < n_f {err:.3e} (bar {bar:.3e}), "
          f"rows that differ at all: {int(np.count_nonzero(np.any(d != 0.0, axis=1)))}")
    assert err <= bar, (err, bar)
    assert np.all(new["Z"][:, K:] == 0.0)


def test_one_tile(legs):
    _check_overlapped(legs, "one_tile", "l48")


def test_ragged_direct_part_l320(legs):
    _check_overlapped(legs, "ragged", "l320")


def test_nothing_to_clear_l160(legs):
    _check_overlapped(legs, "ragged", "l160")


def test_no_panel_to_borrow_q0(legs):
    _check_overlapped(legs, "one_tile", "q0")


def test_declined_tail_is_the_ordinary_path(legs):
    new, old = legs["one_tile"]["decline"], legs["off"]["decline"]
    assert new["tails"] == [0, 0] and old["tails"] == [0, 0], (_small(new), _small(old))
    assert new["overlaps"] == [0, 0] and old["overlaps"] == [0, 0], (_small(new), _small(old))
    assert np.array_equal(new["S"], old["S"], equal_nan=True)
    assert np.array_equal(new["Z"], old["Z"], equal_nan=True)
    assert new["counters"] == old["counters"], (new["counters"], old["counters"])
    assert new["repeat_identical"] and new["bytes_after"] == new["bytes_before"], _small(new)


def test_small_panel_is_left_alone_by_default(legs):
    new, old = legs["default"]["l48"], legs["off"]["l48"]
    assert new["tails"] == [1, 1] and new["overlaps"] == [0, 0], _small(new)
    assert np.array_equal(new["S"], old["S"]) and np.array_equal(new["Z"], old["Z"])
    assert new["counters"] == old["counters"], (new["counters"], old["counters"])
