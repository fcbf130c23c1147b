"""The power step with its interchanges composed on the device and two triangular solves.

Small shapes at the edges of `lowrank_power.hip`: n = 2l (most rows move, many of them more than once), l that is no multiple
of the solves' blocks, a ragged last block, l = N_s - 1 and the path's upper limit of l.  Each case runs the default path and
the GSI_NO_LOWRANK_POWER=1 path in child processes on the same seeded operator and Omega (the switch is read once per
process), with the bars of tests/test_lowrank_power_gpu.py, and compares the check values the step traces
(GSI_LOWRANK_POWER_TRACE=1: max |(P S) C - L| at every LU) with the ones recorded for the build before this one, which formed
C from two explicit inverses (profiles/r09_power_step_check.json): both are rounding noise at the same |C|, so this build's
may not exceed 4 x the earlier one's.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "r09_power_step_check.json")

CHILD = r'''
import json, sys, numpy as np
import gsi_amd as gsi
n, Ns, K, p, q, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
ctx = gsi.Context(0)
op = gsi.lowrank_synthetic_operator(ctx, n, Ns, seed=0, decay=0.75)
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
                               "repeat_identical": same, "finite": bool(np.isfinite(Zh).all() and np.isfinite(Sh).all())}))
'''

# A sample matrix with l - 1 non-zero rows: the panel S (c T) has l columns and rank l - 1, its other rows stay exactly zero
# through the elimination, and the LU meets an exactly zero pivot in its last column.
CHILD_SINGULAR = r'''
import json, sys, numpy as np
import gsi_amd as gsi
n, Ns, K, p, q = 400, 48, 16, 8, 1
rng = np.random.default_rng(5)
samples = np.zeros((Ns, n))
samples[:, 3:3 + K + p - 1] = rng.standard_normal((Ns, K + p - 1))
ctx = gsi.Context(0)
op = gsi.LowRankCovMatrix(samples, ctx)._device_operator()
Om = gsi.DeviceMatrix(ctx, n, K + p).randn(7)
Z = gsi.DeviceMatrix(ctx, n, K + p); S = gsi.DeviceMatrix(ctx, K + p, 1)
code, msg = 0, ""
try:
    gsi._lib.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, S.h), ctx.lib)
except gsi.GsiError as e:
    code, msg = e.code, str(e)
pi = ctx.path_info()
print("result " + json.dumps({"code": code, "msg": msg, "steps": pi["lowrank_power_steps"],
                               "declines": pi["lowrank_power_declines"], "tails": pi["lowrank_tails"]}))
'''

TRACE = re.compile(r"lowrank_power_step: n (\d+) N (\d+) l (\d+), (\d+) moved rows, check max \|\(P S\) C - L\| = (\S+)")


def _run(script, args, power_off, trace=False):
    env = dict(os.environ)
    for k in ("GSI_NO_LOWRANK_TAIL", "GSI_NO_LOWRANK_POWER", "GSI_LOWRANK_POWER_TRACE"):
        env.pop(k, None)
    if power_off:
        env["GSI_NO_LOWRANK_POWER"] = "1"
    if trace:
        env["GSI_LOWRANK_POWER_TRACE"] = "1"
    r = subprocess.run([sys.executable, "-c", script] + [str(a) for a in args], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([s for s in r.stdout.splitlines() if s.startswith("result ")][-1][len("result "):])
    res["trace"] = [(int(m.group(4)), float(m.group(5))) for m in TRACE.finditer(r.stderr)]
    return res


def _child(tmp_path, tag, n, Ns, K, p, q, power_off):
    out = str(tmp_path / tag)
    res = _run(CHILD, [n, Ns, K, p, q, out], power_off, trace=not power_off)
    res["S"] = np.load(out + "_S.npy")
    res["Z"] = np.load(out + "_Z.npy", mmap_mode="r")
    return res


SHAPES = [
    pytest.param(128, 80, 48, 16, 2, id="n-eq-2l"),            # most rows move, a good part of them more than once
    pytest.param(777, 100, 56, 16, 2, id="l72-odd-n"),         # l no multiple of 16 or 32, odd n
    pytest.param(4000, 256, 40, 10, 1, id="l50-ragged"),       # ragged last block of both solves
    pytest.param(3000, 64, 47, 16, 2, id="l-eq-Ns-1"),         # the widest l the path accepts for its N_s
    pytest.param(20000, 512, 320, 64, 1, id="l384"),           # the path's upper limit of l
]


@pytest.mark.parametrize("n,Ns,K,p,q", SHAPES)
def test_power_step_on_the_device_agrees(tmp_path, request, n, Ns, K, p, q):
    new = _child(tmp_path, "power", n, Ns, K, p, q, False)
    old = _child(tmp_path, "off", n, Ns, K, p, q, True)
    info = {k: v for k, v in new.items() if k not in ("S", "Z")}
    assert old["steps"] == 0 and old["declines"] == 0, {k: v for k, v in old.items() if k not in ("S", "Z")}
    assert new["steps_first"] == 2 * q and new["steps"] == 4 * q and new["declines"] == 0, info       # 2q per call
    for r in (new, old):
        assert r["repeat_identical"] and r["finite"] and r["tails"] == 2, {k: v for k, v in r.items() if k not in ("S", "Z")}
    S1, S0 = new["S"], old["S"]
    sv = np.max(np.abs(S1[:K] - S0[:K]) / S0[:K])
    xerr = orc.xis_error_up_to_sign(np.asarray(new["Z"]), np.asarray(old["Z"]), K)
    trace = new["trace"]
    print(f"\n{n} x {Ns}, l = {K + p}, q = {q}: sigma rel-err {sv:.2e}, xi err {xerr:.2e} (relative "
          f"{xerr / np.sqrt(S0[0]):.2e}); moved rows and check values {trace}")
    assert sv <= 1e-13, sv
    assert xerr <= 1e-12 * np.sqrt(S0[0]), (xerr, np.sqrt(S0[0]))
    assert len(trace) == 4 * q and trace[:2 * q] == trace[2 * q:], trace        # one line per LU, the same in both calls
    assert all(0 < m <= 2 * (K + p) for m, _ in trace), trace
    with open(RECORD) as f:
        parent = json.load(f)["shapes"][request.node.callspec.id]["parent"]
    assert len(parent) == 2 * q
    for (_, v), v0 in zip(trace[:2 * q], parent):
        assert v <= 4.0 * v0, (trace, parent)


def test_zero_pivot_declines_as_the_direct_path_reports_it():
    new = _run(CHILD_SINGULAR, [], False)
    old = _run(CHILD_SINGULAR, [], True)
    assert old["code"] == 3 and old["steps"] == 0 and old["declines"] == 0, old      # SingularException from the LU
    assert new["code"] == 3 and new["msg"] == old["msg"], (new, old)                 # the same report, not a NaN result
    assert new["steps"] == 0 and new["declines"] == 1 and new["tails"] == 0, new
