"""randsvd of a LowRankCovMatrix with each panel of a power step factored as two column halves.

Where the power steps run in sample space (section 4.11) and 160 < l <= 320, one-rank randsvd (pipeline.cpp:
randsvd_lowrank_single) factors the left 160 columns of Y = S (c T), forms the right half's Schur complement as S times
N x (l - 160) coefficients (Backend::lowrank_split_schur), factors it below row 160 and hands the joined interchanges to the
power step, whose check covers both halves.  A panel the power step declines is factored again whole.

Each comparison runs the default path and the GSI_NO_LOWRANK_SPLIT=1 path in child processes (the switch is read once per
process) on the same seeded operator and Omega, every child under its own `timeout`, and checks which path ran through
gsi_ctx_path_info.  The bars on sigma and xi are the ones tests/test_lowrank_power_gpu.py applies between its own legs.
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
N_ROWS, N_SAMPLES, PAD = 6000, 400, 16
SIGMA_BAR, XI_BAR = 1e-13, 1e-12          # tests/test_lowrank_power_gpu.py: relative sigma error; xi error over sqrt(sigma_1)
CHILD_SECONDS = 120

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
same = bool(np.array_equal(Zh, Z2, equal_nan=True) and np.array_equal(Sh, S2, equal_nan=True))
np.save(out + "_S.npy", Sh)
np.save(out + "_Z.npy", np.ascontiguousarray(Zh[:, :K]))
print("result " + json.dumps({"split_first": pi1["lowrank_split_lus"], "split": pi["lowrank_split_lus"],
                               "split_declines": pi["lowrank_split_declines"], "steps": pi["lowrank_power_steps"],
                               "declines": pi["lowrank_power_declines"], "tails": pi["lowrank_tails"],
                               "repeat_identical": same, "counters": ctx.counters()}))
'''


def _child(tmp_path, tag, l, q, decay, split_off):
    env = dict(os.environ)
    for k in ("GSI_NO_LOWRANK_TAIL", "GSI_NO_LOWRANK_POWER", "GSI_NO_LOWRANK_SPLIT"):
        env.pop(k, None)
    if split_off:
        env["GSI_NO_LOWRANK_SPLIT"] = "1"
    out = str(tmp_path / tag)
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, "-c", CHILD, str(N_ROWS), str(N_SAMPLES), str(l - PAD),
           str(PAD), str(q), str(decay), out]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    res = json.loads([s for s in r.stdout.splitlines() if s.startswith("result ")][-1][len("result "):])
    res["S"] = np.load(out + "_S.npy")
    res["Z"] = np.load(out + "_Z.npy")
    return res


def _info(r):
    return {k: v for k, v in r.items() if k not in ("S", "Z")}


# l2 = l - 160 = 8 (the narrowest right half), 40 (a ragged block), 160 (the headline's halves)
@pytest.mark.parametrize("l,q", [(168, 1), (200, 1), (320, 1), (320, 2)])
def test_panels_in_two_halves_agree_with_whole_panels(tmp_path, l, q):
    new = _child(tmp_path, "split", l, q, 0.75, False)
    old = _child(tmp_path, "whole", l, q, 0.75, True)
    assert old["split"] == 0 and old["split_declines"] == 0, _info(old)
    assert new["split_first"] == 2 * q and new["split"] == 4 * q and new["split_declines"] == 0, _info(new)     # 2q per call
    for r in (new, old):
        assert r["repeat_identical"], _info(r)
        assert r["steps"] == 4 * q and r["declines"] == 0 and r["tails"] == 2, _info(r)
    K = l - PAD
    S1, S0 = new["S"], old["S"]
    sv = np.max(np.abs(S1[:K] - S0[:K]) / S0[:K])
    xerr = orc.xis_error_up_to_sign(new["Z"], old["Z"], K)
    print(f"\nl = {l}, q = {q}: sigma rel-err {sv:.2e}, xi err {xerr:.2e} (relative {xerr / np.sqrt(S0[0]):.2e})")
    assert sv <= SIGMA_BAR, sv
    assert xerr <= XI_BAR * np.sqrt(S0[0]), (xerr, np.sqrt(S0[0]))


# no right half (l = 160), and a right half wider than the left (l = 330 > 2 * 160)
@pytest.mark.parametrize("l", [160, 330])
def test_widths_outside_the_split_are_factored_whole(tmp_path, l):
    new = _child(tmp_path, "split", l, 1, 0.75, False)
    assert new["split"] == 0 and new["split_declines"] == 0, _info(new)
    assert new["steps"] == 4 and new["declines"] == 0 and new["repeat_identical"], _info(new)


def test_a_declined_panel_is_factored_again_whole_bit_for_bit(tmp_path):
    """Decay 2.5: the power step's check fails at the first LU, for the halves as for the whole panel."""
    new = _child(tmp_path, "split", 320, 1, 2.5, False)
    old = _child(tmp_path, "whole", 320, 1, 2.5, True)
    assert new["split"] == 0 and new["split_declines"] == 2 and new["steps"] == 0 and new["declines"] == 2, _info(new)   # one per call
    assert old["split"] == 0 and old["split_declines"] == 0 and old["steps"] == 0 and old["declines"] == 2, _info(old)
    assert new["repeat_identical"] and old["repeat_identical"]
    assert np.array_equal(new["S"], old["S"], equal_nan=True)
    assert np.array_equal(new["Z"], old["Z"], equal_nan=True)
    assert new["counters"] == old["counters"], (new["counters"], old["counters"])
