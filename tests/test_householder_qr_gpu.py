"""The Householder tier of qr_thinQ (csrc/panel_qr.hip, the Householder branch of HipBackend::qr_thinQ) at its loop edges,
with R and Q pinned to a long-double dlarfg reference.  Cases, references and bars: tests/householder_qr_cases.py;
tests/test_householder_qr_model.py shows with planted defects that every case can fail; tests/test_householder_qr_cpu.py
runs the same checks on LAPACK and on the CPU reference library.  Nothing stands behind this tier: it takes what the two
CholeskyQR tiers refuse (m < 2 l, l > 1024, condition beyond ~1e13, exact rank deficiency), and a wrong Q here is returned.

kernel -> edge -> case that reaches it
  qr_step_kernel           thread = one row, 256-row workgroups, rows_per_thread sweeps, nlive = live panel columns
    one workgroup, fewer rows than threads          1x1 2x1 5x5 16x16 17x17 33x32 100x60
    one row in the last workgroup                   257x31 (j = 0), 513x33 (j = 0: third workgroup)
    rows <= 0 after the last column (break)         16x16 17x17 5x5 1x1: m == l
    rows_per_thread == 2, second sweep of one row   262145x17 (and `part` sized by qr_max_blocks)
    panel width 15, 16, 1, 4, 9                     300x15, 300x16, 300x17 / 513x33 / 1100x1025 (b = 1), 4400x20, 300x41graded
  qr_house_kernel          16-way fixed-order sum of the workgroup partials, dlarfg, row j of R, the next coefficients
    one trip of the partial sum                     every case below 4097 rows
    second trip (p = g + 16): 18 workgroups         4400x20, 4400x20graded; 1025 workgroups over 512 rows: 262145x17
    sigma == 0 (H = I, tau = 0)                     upper40x20 (every step), m == l (last step), the zero column of
                                                    2000x40rank7zerocol (alpha == 0 too), signed40x20 where the +-1 sits
                                                    on the diagonal
  qr_copyV / G = V'V / qr_buildT / qr_applyT        T' in the trailing update, T in forming Q, last panel first
    no trailing update                              l <= 16
    one, two, 64 trailing updates                   l = 17 .. 32; 33, 41, 60; 1100x1025
  range guard (qr_absmax, qr_scale)                 300x33 times 2^+-400 (just outside the window: equal bits), 2^+-520, 2^+-600
  tier gate, no switch set                          100x60 (m < 2 l), 1100x1025 (l > 1024), the rank-deficient panels (both
                                                    CholeskyQR tiers decline)
Every other full-rank case needs GSI_NO_CHOLQR, which is read once per process: they all run in ONE child process, each on a
fresh context, and the parent checks what the child wrote.  Every case asserts the counter deltas of its context.

Exact cases (np.array_equal): [U; 0] -> R == U, Q == [I; 0]; one +-1 per column in distinct rows -> Q R == Y, Q'Q == I, every
entry in {0, +-1} (600x33: the rows lie beyond the first workgroup); qr(2^s Y) == (Q, 2^s R) for s = +-300, +-400; two runs
of 4400x20 on one context.

Range: for 2^+-520 Y and 2^+-600 Y the call must raise GsiError or meet every full-rank bar.  A build of the library without
the range guard, run through these four tests on the MI355X, returned status 0 with non-finite factors at 2^+520 and 2^+600,
with |Q'Q - I|max = 1.8e-12 (17.9 of the bar; resid 920, R 202, Q 189 of theirs) at 2^-520 and with Q = [I; 0] (resid 1.2e14
of the bar) at 2^-600 -- the figures of the restatement with `no_prescale`, digit for digit.  With the guard (DESIGN.md 4.3:
exact prescale outside [2^-400, 2^400]) the device meets the bars at all four scales, with the ratios of the unscaled panel.

Largest ratio measured / bar per bar (householder_qr_cases.py states the bars; "CPU" is the CPU reference library, "HIP" what
this module measured on an MI355X: profiles/householder_qr_errors.json, written by a run with HHQR_RECORD=<path>):
             orth              resid                  R                     Q                  range
  LAPACK     0.014 (300x41g)   0.22 (5x5)             0.047 (2x1)           0.046 (262145x17)  4.6e-5 (2000x40rank7)
  CPU        0.24 (262145x17)  0.58 (2000x40rank7)    2.58 (262145x17) *    0.080 (300x16)     2.5e-4 (2000x40rank7)
  model      0.018 (1100x1025) 0.44 (rank7zerocol)    0.066 (300x16)        0.055 (262145x17)  6.2e-5 (300x12rank5)
  HIP        0.016 (300x41g)   0.17 (17x17)           0.055 (2x1)           0.055 (262145x17)  4.1e-5 (300x12rank5)
  * the CPU library sums 262145 terms one after the other; its bar alone carries sqrt(m) for that case
    (tests/test_householder_qr_cpu.py says why).  No bar is widened for HIP.
Wall time of this module on the MI355X: 5 s, 32 tests (the long-double reference of 262145x17 is the longest host step).

Out of scope: leading dimensions other than m (gsi_qr_thinQ always passes ld == m); the stacked-R paths of several ranks;
svd_tall behind a Householder QR (test_jacobi_svd_gpu.py); per-column extremes of range.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import householder_qr_cases as hc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TIERS = ("cholqr2", "scholqr3", "householder")
RECORD_ENV = "HHQR_RECORD"
RERUN = hc.FORCED[11]                  # 4400x20: twice on one context


def _deltas(before, after):
    return [after[k] - before[k] for k in TIERS]


# ---- the child: every forced case, one process, GSI_NO_CHOLQR set ------------------------------------------------------
def child_main(out):
    """Every case that needs the switch, each on a fresh context; results to `out` (.npz).  The first exception from the
    library that is not a refusal of a range case ends the child: nothing is launched after it."""
    import gsi_amd as gsi
    res = {}

    def run(key, Y, ctx=None):
        c = ctx or gsi.Context(0)
        try:
            before = c.counters()
            Q, R = gsi.qr_thinQ(Y, return_R=True, ctx=c)
            res["d_" + key] = np.array(_deltas(before, c.counters()))
            res["Q_" + key], res["R_" + key] = Q, R
        finally:
            if ctx is None:
                c.close()

    for case in hc.FORCED:
        run(case.name, hc.panel(case))
    for name in hc.EXACT:
        run(name, exact_panel(name))
    Y = hc.panel(hc.SCALE_BASE)
    run("base", Y)
    for s in hc.SCALINGS:
        run("scale%+d" % s, np.asfortranarray(np.ldexp(Y, s)))
    for s in hc.RANGES:
        try:
            run("range%+d" % s, np.asfortranarray(np.ldexp(Y, s)))
        except gsi.GsiError as e:
            if e.code != 1:                              # only an argument error that names the range is a refusal
                raise
            res["raised_range%+d" % s] = np.array(str(e))
    c = gsi.Context(0)
    try:
        run("again1", hc.panel(RERUN), ctx=c)
        run("again2", hc.panel(RERUN), ctx=c)
    finally:
        c.close()
    np.savez(out, **res)
    print("hhqr-ok", flush=True)


def exact_panel(name):
    if name == "upper40x20":
        return hc.upper_triangular_panel()[0]
    return hc.signed_selection_panel(40, 20) if name == "signed40x20" else hc.signed_selection_panel(600, 33, first_row=256)


_CODE = ("import sys\n"
         "sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
         "import test_householder_qr_gpu as t\n"
         "t.child_main(sys.argv[3])\n")


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hhqr") / "forced.npz")
    env = dict(os.environ)
    env["GSI_NO_CHOLQR"] = "1"
    env.pop(RECORD_ENV, None)
    r = subprocess.run([sys.executable, "-c", _CODE, ROOT, HERE, out], capture_output=True, text=True, timeout=600, env=env,
                       cwd=ROOT)
    assert r.returncode == 0 and "hhqr-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.fixture(scope="module", autouse=True)
def record():
    t0 = time.time()
    yield
    path = os.environ.get(RECORD_ENV)
    hip = hc.MEASURED.get("hip", {})
    if path and hip:
        worst = {}
        for name, ratios in hip.items():
            for bar, v in ratios.items():
                if v >= worst.get(bar, {"ratio": -1.0})["ratio"]:
                    worst[bar] = {"ratio": v, "case": name}
        with open(path, "w") as f:
            json.dump({"what": "measured / bar on the MI355X, tests/test_householder_qr_gpu.py; bars in tests/householder_qr_cases.py",
                       "module_wall_seconds": round(time.time() - t0, 1), "largest_per_bar": worst, "per_case": hip}, f, indent=1)


class Refused(Exception):
    pass


def stored(forced, key):
    """The child's factors for `key` as a qr callable (the panel is regenerated from the same seed on both sides)."""
    def qr(Y):
        if "raised_" + key in forced.files:
            raise Refused(str(forced["raised_" + key]))
        return forced["Q_" + key], forced["R_" + key]
    return qr


def householder_only(forced, key):
    assert forced["d_" + key].tolist() == [0, 0, 1], (key, dict(zip(TIERS, forced["d_" + key].tolist())))


# ---- forced cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.FORCED, ids=lambda c: c.name)
def test_forced_table(forced, case):
    householder_only(forced, case.name)
    hc.check_case(stored(forced, case.name), case, who="hip")


@pytest.mark.parametrize("name", hc.EXACT)
def test_exact(forced, name):
    householder_only(forced, name)
    hc.check_exact(stored(forced, name), name)


@pytest.mark.parametrize("s", hc.SCALINGS)
def test_scaling_equal_bits(forced, s):
    key = "scale%+d" % s
    householder_only(forced, "base")
    householder_only(forced, key)
    hc.check_scaling(stored(forced, key), s, base=(forced["Q_base"], forced["R_base"]))


@pytest.mark.parametrize("s", hc.RANGES)
def test_range_raises_or_meets_the_bars(forced, s):
    key = "range%+d" % s
    ratios = hc.check_range(stored(forced, key), s, (Refused,), who="hip")
    if ratios is None:
        assert "range" in str(forced["raised_" + key]).lower()
    else:
        householder_only(forced, key)


def test_run_to_run_equal_bits(forced):
    householder_only(forced, "again1")
    householder_only(forced, "again2")
    assert np.array_equal(forced["Q_again1"], forced["Q_again2"])
    assert np.array_equal(forced["R_again1"], forced["R_again2"])
    assert np.array_equal(forced["Q_again1"], forced["Q_" + RERUN.name])
    assert np.array_equal(forced["R_again1"], forced["R_" + RERUN.name])


# ---- gate cases: no switch, a fresh context each ------------------------------------------------------------------------------
def run_fresh(gsi, Y):
    c = gsi.Context(0)
    try:
        before = c.counters()
        Q, R = gsi.qr_thinQ(Y, return_R=True, ctx=c)
        return Q, R, dict(zip(TIERS, _deltas(before, c.counters())))
    finally:
        c.close()


@pytest.mark.parametrize("case", hc.GATE, ids=lambda c: c.name)
def test_gate_closed(gsi, case):
    seen = {}

    def qr(Y):
        Q, R, seen["d"] = run_fresh(gsi, Y)
        return Q, R
    hc.check_case(qr, case, who="hip")
    assert seen["d"] == {"cholqr2": 0, "scholqr3": 0, "householder": 1}, seen


@pytest.mark.parametrize("case", hc.RANKDEF, ids=lambda c: c.name)
def test_rank_deficient_reaches_householder(gsi, case):
    seen = {}

    def qr(Y):
        Q, R, seen["d"] = run_fresh(gsi, Y)
        return Q, R
    hc.check_case(qr, case, who="hip")
    assert seen["d"]["householder"] == 1, seen
