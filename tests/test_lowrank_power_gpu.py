"""randsvd of a LowRankCovMatrix with the range finder's power steps in sample space.

After each panel LU of Y = c S T, one-rank randsvd (pipeline.cpp: randsvd_lowrank_single) forms
T_next = S'L = G C + S[mv]'((S[perm(mv)] - S[mv]) C) with
C = c T U^-1 (Backend::lowrank_power_step) instead of the n x l product S'L; the check of (P S) C against the L in memory
declines where the coefficients no longer reproduce L, and that call goes on with the direct path.

Each comparison runs the default path and the GSI_NO_LOWRANK_POWER=1 path (tail still on) in child processes (the switch
is read once per process) on the same seeded operator and Omega, and checks which path ran through gsi_ctx_path_info.
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
pi1 = ctx.path_info()
Z2, S2 = run()
pi = ctx.path_info()
same = bool(np.array_equal(Zh, Z2) and np.array_equal(Sh, S2))
np.save(out + "_S.npy", Sh)
np.save(out + "_Z.npy", np.ascontiguousarray(Zh[:, :K]))
print("result " + json.dumps({"steps_first": pi1["lowrank_power_steps"], "steps": pi["lowrank_power_steps"],
                               "declines": pi["lowrank_power_declines"], "tails": pi["lowrank_tails"],
                               "repeat_identical": same, "counters": ctx.counters()}))
'''


def _child(tmp_path, tag, n, Ns, K, p, q, decay, power_off):
    env = dict(os.environ)
    env.pop("GSI_NO_LOWRANK_TAIL", None)
    env.pop("GSI_NO_LOWRANK_POWER", None)
    if power_off:
        env["GSI_NO_LOWRANK_POWER"] = "1"
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", CHILD, str(n), str(Ns), str(K), str(p), str(q), str(decay), out],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([s for s in r.stdout.splitlines() if s.startswith("result ")][-1][len("result "):])
    res["S"] = np.load(out + "_S.npy")
    res["Z"] = np.load(out + "_Z.npy", mmap_mode="r")
    return res


# the AGREE shapes of tests/test_lowrank_tail_gpu.py that have power steps (q >= 1)
AGREE = [
    pytest.param(1000000, 1024, 256, 64, 2, 0.75, id="headline-1e6"),
    pytest.param(200000, 1024, 256, 64, 1, 0.75, id="2e5-q1"),
    pytest.param(200000, 1024, 256, 64, 3, 0.75, id="2e5-q3"),
    pytest.param(5000, 512, 32, 16, 2, 0.75, id="5000-l48"),
]


@pytest.mark.parametrize("n,Ns,K,p,q,decay", AGREE)
def test_power_steps_in_sample_space_agree(tmp_path, n, Ns, K, p, q, decay):
    new = _child(tmp_path, "power", n, Ns, K, p, q, decay, False)
    old = _child(tmp_path, "off", n, Ns, K, p, q, decay, True)
    assert old["steps"] == 0 and old["declines"] == 0, old
    info = {k: v for k, v in new.items() if k not in ("S", "Z")}
    assert new["steps_first"] == 2 * q and new["steps"] == 4 * q and new["declines"] == 0, info   # 2q per call
    for r in (new, old):
        assert r["repeat_identical"], {k: v for k, v in r.items() if k not in ("S", "Z")}
        assert r["tails"] == 2, r["tails"]
    for k in ("cholqr2", "householder", "scholqr3"):                 # (Jacobi sweeps may differ with the rounding)
        assert new["counters"][k] == old["counters"][k], (new["counters"], old["counters"])
    S1, S0 = new["S"], old["S"]
    sv = np.max(np.abs(S1[:K] - S0[:K]) / S0[:K])
    xerr = orc.xis_error_up_to_sign(np.asarray(new["Z"]), np.asarray(old["Z"]), K)
    print(f"\n{n} x {Ns}, l = {K + p}, q = {q}: sigma rel-err {sv:.2e}, xi err {xerr:.2e} (relative {xerr / np.sqrt(S0[0]):.2e})")
    assert sv <= 1e-13, sv
    assert xerr <= 1e-12 * np.sqrt(S0[0]), (xerr, np.sqrt(S0[0]))


# the power steps must decline (decay 2.5: the check of L fails at the first LU) or not run at all (l >= N_s)
DECLINE = [
    pytest.param(100000, 1024, 256, 64, 2, 2.5, 1, id="decay2.5"),
    pytest.param(5000, 64, 48, 16, 2, 0.75, 0, id="l-eq-Ns"),
    pytest.param(5000, 64, 56, 16, 1, 0.75, 0, id="l-gt-Ns"),
]


@pytest.mark.parametrize("n,Ns,K,p,q,decay,declines_per_call", DECLINE)
def test_power_steps_decline_bit_identically(tmp_path, n, Ns, K, p, q, decay, declines_per_call):
    new = _child(tmp_path, "power", n, Ns, K, p, q, decay, False)
    old = _child(tmp_path, "off", n, Ns, K, p, q, decay, True)
    assert new["steps"] == 0 and new["declines"] == 2 * declines_per_call, {k: v for k, v in new.items() if k not in ("S", "Z")}
    assert old["steps"] == 0 and old["declines"] == 0
    assert new["repeat_identical"] and old["repeat_identical"]
    assert np.array_equal(new["S"], old["S"], equal_nan=True)
    assert np.array_equal(np.asarray(new["Z"]), np.asarray(old["Z"]), equal_nan=True)
    assert new["counters"] == old["counters"], (new["counters"], old["counters"])
