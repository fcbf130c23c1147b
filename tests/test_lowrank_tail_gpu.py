"""randsvd of a LowRankCovMatrix with its tail in sample space.

After the last panel LU L, one-rank randsvd of A = S S' / (N - 1) (pipeline.cpp: randsvd_lowrank_single) has T = S'L and
finishes on N x l coefficient matrices (Backend::lowrank_tail): CholeskyQR2 of Y = A L and of W = A'Q through M'(G M) with
the sample Gram matrix G = S'S cached on the operator, the l x l SVD, and one tall product Z = S C.  Where it declines (a Cholesky breakdown, a failed orthogonality
check, l > N - 1) the ordinary path runs from the same T, bit for bit.

Each comparison runs the sample-space path and the GSI_NO_LOWRANK_TAIL=1 path in child processes (the switch is read once
per process) on the same seeded operator and Omega, and checks which path ran through gsi_ctx_path_info.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys, numpy as np
import gsi_amd as gsi
n, Ns, K, p, q, decay, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6]), sys.argv[7]
ctx = gsi.Context(0)
op = gsi.lowrank_synthetic_operator(ctx, n, Ns, seed=0, decay=decay)
Om = gsi.DeviceMatrix(ctx, n, K + p).randn(7)
Z = gsi.DeviceMatrix(ctx, n, K + p); S = gsi.DeviceMatrix(ctx, K + p, 1)
def run():
    gsi._lib.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, S.h), ctx.lib)
    return Z.to_host(), S.to_host()[:, 0]
Zh, Sh = run()
tails1 = ctx.path_info()["lowrank_tails"]
Z2, S2 = run()                                          # the second call reuses the operator's Gram matrix
same = bool(np.array_equal(Zh, Z2) and np.array_equal(Sh, S2))
np.save(out + "_S.npy", Sh)
np.save(out + "_Z.npy", np.ascontiguousarray(Zh[:, :K]))
print("result " + json.dumps({"tails_first": tails1, "tails": ctx.path_info()["lowrank_tails"], "repeat_identical": same,
                               "zero_tail": bool(np.all(Zh[:, K:] == 0.0)), "counters": ctx.counters()}))
'''


def _child(tmp_path, tag, n, Ns, K, p, q, decay, tail_off):
    env = dict(os.environ)
    env.pop("GSI_NO_LOWRANK_TAIL", None)
    if tail_off:
        env["GSI_NO_LOWRANK_TAIL"] = "1"
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", CHILD, str(n), str(Ns), str(K), str(p), str(q), str(decay), out],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([s for s in r.stdout.splitlines() if s.startswith("result ")][-1][len("result "):])
    res["S"] = np.load(out + "_S.npy")
    res["Z"] = np.load(out + "_Z.npy", mmap_mode="r")
    return res


def _pair(tmp_path, n, Ns, K, p, q, decay):
    new = _child(tmp_path, "tail", n, Ns, K, p, q, decay, False)
    old = _child(tmp_path, "off", n, Ns, K, p, q, decay, True)
    assert old["tails"] == 0
    for r in (new, old):
        assert r["repeat_identical"] and r["zero_tail"], {k: v for k, v in r.items() if k not in ("S", "Z")}
        assert r["counters"]["householder"] == 0, r["counters"]
    return new, old


# (n, N_s, K, p, q, decay): the headline size, a synthetic operator at l = 320 with q = 0, 1, 3, a small one at l = 48
AGREE = [
    pytest.param(1000000, 1024, 256, 64, 2, 0.75, id="headline-1e6"),
    pytest.param(200000, 1024, 256, 64, 0, 0.75, id="2e5-q0"),
    pytest.param(200000, 1024, 256, 64, 1, 0.75, id="2e5-q1"),
    pytest.param(200000, 1024, 256, 64, 3, 0.75, id="2e5-q3"),
    pytest.param(5000, 512, 32, 16, 2, 0.75, id="5000-l48"),
]


@pytest.mark.parametrize("n,Ns,K,p,q,decay", AGREE)
def test_sample_space_tail_agrees(tmp_path, n, Ns, K, p, q, decay):
    new, old = _pair(tmp_path, n, Ns, K, p, q, decay)
    assert new["tails_first"] == 1 and new["tails"] == 2, new         # both calls finished in sample space
    # each call: the CholeskyQR2 of Y and of W, as on the ordinary path
    assert new["counters"]["cholqr2"] == 4 and new["counters"]["householder"] == 0, new["counters"]
    S1, S0 = new["S"], old["S"]
    sv = np.max(np.abs(S1[:K] - S0[:K]) / S0[:K])
    assert sv <= 1e-13, sv
    # xi_i = v_i sqrt(sigma_i): the distance up to sign relative to the longest column, sqrt(sigma_1) (an absolute 1e-12 is
    # 1.4e-12 at q = 0, n = 2e5, where the sketch separates the trailing sigma_i less and both paths' vectors move with it)
    xerr = orc.xis_error_up_to_sign(np.asarray(new["Z"]), np.asarray(old["Z"]), K)
    print(f"\n{n} x {Ns}, l = {K + p}, q = {q}: sigma rel-err {sv:.2e}, xi err {xerr:.2e} (relative {xerr / np.sqrt(S0[0]):.2e})")
    assert xerr <= 1e-12 * np.sqrt(S0[0]), (xerr, np.sqrt(S0[0]))


# the tail must decline: a spectrum too steep for a first CholeskyQR round (decay 2.5), and l >= N_s (Y rank-deficient)
DECLINE = [
    pytest.param(100000, 1024, 256, 64, 2, 2.5, id="decay2.5"),
    pytest.param(5000, 64, 48, 16, 2, 0.75, id="l-eq-Ns"),
    pytest.param(5000, 64, 56, 16, 1, 0.75, id="l-gt-Ns"),
]


@pytest.mark.parametrize("n,Ns,K,p,q,decay", DECLINE)
def test_sample_space_tail_declines_bit_identically(tmp_path, n, Ns, K, p, q, decay):
    new = _child(tmp_path, "tail", n, Ns, K, p, q, decay, False)
    old = _child(tmp_path, "off", n, Ns, K, p, q, decay, True)
    assert new["tails"] == 0 and old["tails"] == 0, (new["tails"], old["tails"])
    assert np.array_equal(new["S"], old["S"], equal_nan=True)
    assert np.array_equal(np.asarray(new["Z"]), np.asarray(old["Z"]), equal_nan=True)
    assert new["counters"] == old["counters"], (new["counters"], old["counters"])


def test_sample_gram_is_freed_with_the_operator(gsi):
    """The Gram matrix lives as long as its operator: closing the operator gives device_bytes() back (the cache emptied
    both times; workspaces of the shapes involved exist before the measured window)."""
    ctx = gsi.Context(0)
    try:
        n, Ns, K, p, q = 20000, 512, 48, 16, 1
        Om = gsi.DeviceMatrix(ctx, n, K + p).randn(3)
        Z = gsi.DeviceMatrix(ctx, n, K + p)
        S = gsi.DeviceMatrix(ctx, K + p, 1)

        def run(op):
            gsi._lib.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, S.h), ctx.lib)

        warm = gsi.lowrank_synthetic_operator(ctx, n, Ns, seed=1, decay=0.75)
        run(warm)
        warm.close()
        ctx.release_cache()
        before = ctx.device_bytes()
        op = gsi.lowrank_synthetic_operator(ctx, n, Ns, seed=2, decay=0.75)
        tails = ctx.path_info()["lowrank_tails"]
        run(op)
        assert ctx.path_info()["lowrank_tails"] == tails + 1
        ctx.release_cache()
        held = ctx.device_bytes()
        assert held >= before + 8 * (Ns * Ns + n * Ns), (held, before)        # the samples and G, while the operator lives
        op.close()
        ctx.release_cache()
        assert ctx.device_bytes() == before, (ctx.device_bytes(), before)
        for h in (Om, Z, S):
            h.close()
    finally:
        ctx.close()
