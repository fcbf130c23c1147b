"""The single-rank panel LU under block schedules other than uniform 64 (csrc/lu_schedule.hpp, panel_lu_blocks.hip).

Every element of L accumulates its k terms in ascending order, in groups of four, wherever a block ends, so a
forced schedule (GSI_LU_SCHEDULE), the chooser's own pick and uniform 64-column blocks (GSI_LU_NB=64) must give the same bits,
and the pivots must be dgetrf's (scipy.linalg.lu_factor).  Panels: 5000 rows with the far-apart ties of
tests/test_lu_leftlook_gpu.py at l = 56, 112, 160, 168, 320, and one of 9 l rows.  The lists at l = 160 are the ones the
schedule was chosen among; at the other widths every width 16, 32, 48, 64 stands first, in the middle and last at least once,
the last block is ragged at l = 56 and 168, and l = 320 has more than 256 finished columns to the left of its last blocks
(two left-looking launches).  The knobs are read at every factorization; each test sets them in a child process of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg

from test_lu_leftlook_gpu import _panel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 120

L160 = [(48, 48, 64), (64, 48, 48), (32, 32, 48, 48), (16, 48, 64, 32)]
CASES = {
    (5000, 56): [(16, 40), (48, 8), (32, 24), (16, 16, 16, 8)],
    (5000, 112): [(48, 64), (64, 48), (16, 32, 48, 16), (48, 48, 16), (32, 16, 64)],
    (5000, 160): L160,
    (5000, 168): [(48, 48, 64, 8), (64, 48, 48, 8), (32, 32, 48, 48, 8), (16, 48, 64, 40)],
    (5000, 320): [(48, 48, 64, 48, 48, 64), (64, 48, 48, 64, 48, 48), (32, 32, 48, 48) * 2, (16, 48, 64, 32) * 2],
    (9 * 160, 160): L160,
}

CHILD = r'''
import ctypes as C, json, os, sys, numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import gsi_amd as gsi
from test_lu_leftlook_gpu import _panel
m, l, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
lists = json.loads(sys.argv[4])
ctx = gsi.Context(0)
Y = _panel(m, l, True)
def schedule():
    w = (C.c_int32 * ((l + 15) // 16))(); n = C.c_int32(0)
    assert ctx.lib.gsi_lu_schedule(l, w, C.byref(n)) == 0
    return [int(w[i]) for i in range(n.value)]
res, ran = {}, []
def factor(tag, env):
    for k in ("GSI_LU_SCHEDULE", "GSI_LU_NB"):
        os.environ.pop(k, None)
    os.environ.update(env)
    ran.append(schedule())
    L, piv = gsi.lu_L(Y, return_pivots=True, ctx=ctx)
    res["L_" + tag], res["p_" + tag] = L, piv
factor("uniform", {"GSI_LU_NB": "64"})
factor("chosen", {})
for i, w in enumerate(lists):
    factor("forced%d" % i, {"GSI_LU_SCHEDULE": ",".join(str(s) for s in w)})
np.savez(out, **res)
print("result " + json.dumps(ran))
'''


def _run(tmp_path, m, l, lists):
    env = dict(os.environ)
    for k in ("GSI_LU_SCHEDULE", "GSI_LU_NB", "GSI_LU_TALL"):
        env.pop(k, None)
    out = str(tmp_path / "lu.npz")
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, "-c", CHILD, str(m), str(l), out, json.dumps(lists)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    ran = json.loads([s for s in r.stdout.splitlines() if s.startswith("result ")][-1][len("result "):])
    return np.load(out), ran


def test_the_lists_cover_every_width_in_every_place():
    others = [w for (m, l), ws in CASES.items() if l != 160 for w in ws]
    for s in (16, 32, 48, 64):
        assert any(w[0] == s for w in others) and any(w[-1] == s for w in others), s
        assert any(s in w[1:-1] for w in others), s
    assert any(w[-1] % 16 for w in others)
    for (m, l), ws in CASES.items():
        assert all(sum(w) == l for w in ws), (m, l)


@pytest.mark.parametrize("m,l", sorted(CASES))
def test_forced_and_chosen_schedules_equal_uniform_64_bit_for_bit(tmp_path, m, l):
    lists = [list(w) for w in CASES[(m, l)]]
    res, ran = _run(tmp_path, m, l, lists)
    assert ran[0] == [min(64, l - jb) for jb in range(0, l, 64)], ran[0]
    assert ran[2:] == lists, ran                      # every forced list is the one that ran
    Y = _panel(m, l, True)
    piv_ref = scipy.linalg.lu_factor(Y)[1]
    assert np.array_equal(res["p_uniform"], piv_ref)
    for tag in ["chosen"] + ["forced%d" % i for i in range(len(lists))]:
        assert np.array_equal(res["p_" + tag], piv_ref), (tag, ran)
        assert np.array_equal(res["L_" + tag], res["L_uniform"]), (tag, ran)


RANDSVD_CHILD = r'''
import json, os, sys, numpy as np
import gsi_amd as gsi
n, Ns, K, p, q = (int(a) for a in sys.argv[1:6])
out = sys.argv[6]
ctx = gsi.Context(0)
op = gsi.lowrank_synthetic_operator(ctx, n, Ns, seed=0, decay=0.75)
Om = gsi.DeviceMatrix(ctx, n, K + p).randn(7)
Z = gsi.DeviceMatrix(ctx, n, K + p); S = gsi.DeviceMatrix(ctx, K + p, 1)
info = {}
for tag, env in (("uniform", {"GSI_LU_NB": "64"}), ("chosen", {})):
    for k in ("GSI_LU_SCHEDULE", "GSI_LU_NB"):
        os.environ.pop(k, None)
    os.environ.update(env)
    before = ctx.path_info()["lowrank_split_lus"]
    gsi._lib.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, S.h), ctx.lib)
    info[tag] = ctx.path_info()["lowrank_split_lus"] - before
    np.save(out + "_S_" + tag + ".npy", S.to_host()[:, 0])
    np.save(out + "_Z_" + tag + ".npy", np.ascontiguousarray(Z.to_host()[:, :K]))
print("result " + json.dumps(info))
'''


def test_randsvd_in_two_halves_equals_uniform_64_bit_for_bit(tmp_path):
    """n = 6000, N_s = 400, l = 320, q = 2 (tests/test_lowrank_split_gpu.py's shape): every LU is two 160-column halves."""
    env = dict(os.environ)
    for k in ("GSI_LU_SCHEDULE", "GSI_LU_NB", "GSI_LU_TALL", "GSI_NO_LOWRANK_TAIL", "GSI_NO_LOWRANK_POWER", "GSI_NO_LOWRANK_SPLIT"):
        env.pop(k, None)
    out = str(tmp_path / "rs")
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, "-c", RANDSVD_CHILD, "6000", "400", "304", "16", "2", out]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    info = json.loads([s for s in r.stdout.splitlines() if s.startswith("result ")][-1][len("result "):])
    assert info == {"uniform": 4, "chosen": 4}, info          # both legs factored their panels in halves
    for what in ("S", "Z"):
        a, b = np.load(out + "_%s_uniform.npy" % what), np.load(out + "_%s_chosen.npy" % what)
        assert np.array_equal(a, b), what
