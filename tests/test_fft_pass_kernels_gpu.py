"""Every reachable fft_pass_kernel<MODE, LR, SHORT> instantiation (csrc/fft_cov.hip) against an exact integer reference.

Operator: fft_gridcov_operator(Ns, table=tab), nugget = 0, tab integer in [-3, 3]; X integer in [-4, 4].  The implied matrix
A[i, j] = tab[|i0 - j0|, |i1 - j1|, |i2 - j2|] and Y_ref = A X are integer, every partial sum far below 2^53, so the
float64 reference (fft_pass_model.exact_reference) is exact in any summation order and carries no error of its own: a wrong
index, stride, line, pair, column or spectrum offset moves an entry of Y by an integer.  A random table has no symmetry
beyond evenness along each axis, so a transposed spectrum offset on a square embedding cannot cancel.  (The header allows
any table: only its restriction to the box is used, positive definiteness is not required.)

Bar: max|Y - Y_ref| <= 1e-12 max|Y_ref| for op.matmul and op.rmatmul_t, the bar the project applies to this operator
(test_fft_gridcov_gpu.py).  It is of the order of the worst case: Higham's bound is log2(Mtot) eta per transform, eta ~ 36 eps
here (the kernel builds W^r from a two-table product and up to three squarings: ~30 eps of twiddle error), two
transforms: ~2e-13 at 8192 embedding points.  numpy's double FFT of the same embedding stays below 4e-16 on every case
(test_fft_pass_model.py asserts the bar for it where n <= 4096).

Which launches a case reaches is decided by tests/fft_pass_model.py (a host model of fft_cov_apply / fft_pass /
launch_pass and the plan's pairs-per-batch rule), and test_fft_pass_model.py proves on the CPU that the table reaches all
36 instantiations, every line length, both layouts, both s_lin branches, ragged and full tiles, both forms of off(),
persistent loops with several pairs, both item orders and a second pair batch in every dimension.

Coverage (MODE<LR, S|L>Ma: S = SHORT; /T = lines per strided tile; !lin = the clamped fill; * = the workgroups loop
whatever the occupancy; rag = ragged last axis-0 tile; the inverse passes 25 / 16 mirror 3 / 0; MODE 15 = 1-D fused,
3 / 25 = axis 0 forward / inverse, 0 / 16 = middle axis forward / inverse, 4 = fused last axis):

  1-D            (2,)1 15<2,S>4   (3,)2 (4,)3 15<3,S>8   (7,)3 15<0,L>16   (13,)2 15<1,L>32   (31,)5 15<2,L>64   (50,)7 15<3,L>128
                 (100,)3 15<0,L>256   (200,)2 15<1,L>512   (300,)3 15<2,L>1024   (600,)131 15<3,L>2048, batches of 64 + 2 pairs
                 (1500,)3 15<0,L>4096   (4096,)3 15<1,L>8192
  2-D natural    (2,5)3     3<2,S>4      4<0,L>16/T4!lin        (3,9)2     3<3,S>8     4<1,L>32/T8!lin
                 (5,2)3     3<0,L>16     4<2,S>4/T16!lin        (9,3)5     3<1,L>32    4<3,S>8/T16!lin
                 (17,17)131 3<2,L>64     4<2,L>64/T16  64 + 2 pairs, odd last column, square embedding
                 (33,40)7   3<3,L>128    4<3,L>128/T16 rag      (4,70)3    3<3,S>8     4<0,L>256/T8 rag
                 (6,130)2   3<0,L>16     4<1,L>512/T16 rag      (3,1100)3  3<3,S>8     4<0,L>4096/T2 rag
                 (2,2049)2  3<2,S>4      4<1,L>8192/T1 rag      (5,600)3   3<0,L>16    4<3,L>2048/T4 rag
  2-D blocked    (65,2)3    3<0,L>256    4<2,S>4/T16!lin        (130,7)5   3<1,L>512   4<0,L>16/T16!lin
                 (300,3)2   3<2,L>1024   4<3,S>8/T16!lin        (600,20)3  3<3,L>2048  4<2,L>64/T16
                 (1100,3)1  3<0,L>4096   4<3,S>8/T16!lin        (2049,2)3  3<1,L>8192  4<2,S>4/T16!lin
                 (70,300)19 3<0,L>256    4<2,L>1024/T8* 512 threads, 320 items, 10 pairs, rag
                 (66,600)1  3<0,L>256    4<3,L>2048/T4 rag
                 (300,33)131 3<2,L>1024* 4<3,L>128/T16* 576 axis-0 items of 256 threads, rag; 64 + 2 pairs, odd last column
                 (2049,9)59 3<1,L>8192*  4<1,L>32/T16*  eight waves per line, 270 items, 30 pairs
  3-D natural    (3,2,5)3   3<3,S>8  0<2,S>4/T8!lin   4<0,L>16/T16!lin     (5,3,2)2   3<0,L>16 0<3,S>8/T16!lin 4<2,S>4/T16!lin
                 (2,5,9)3   3<2,S>4  0<0,L>16/T4!lin  4<1,L>32/T16 rag     (4,9,3)3   3<3,S>8  0<1,L>32/T8!lin 4<3,S>8/T16!lin
                 (6,17,4)5  3<0,L>16 0<2,L>64/T16     4<3,S>8/T16!lin rag  (3,40,5)2  3<3,S>8  0<3,L>128/T8    4<0,L>16/T16!lin rag
                 (3,70,5)3  3<3,S>8  0<0,L>256/T8     4<0,L>16/T16!lin rag
                 (9,6,11)131 3<1,L>32 0<0,L>16/T16!lin 4<1,L>32/T16 rag; 64 + 2 pairs, odd last column
                 (2,130,3)2 3<2,S>4  0<1,L>512/T4     4<3,S>8/T16!lin rag  (2,300,2)1 3<2,S>4  0<2,L>1024/T4   4<2,S>4/T16!lin rag
                 (2,600,2)2 3<2,S>4  0<3,L>2048/T4    4<2,S>4/T16!lin rag  (2,1100,2)1 3<2,S>4 0<0,L>4096/T2   4<2,S>4/T16!lin rag
                 (9,130,9)29 3<1,L>32 0<1,L>512/T16* 4<1,L>32/T16* 512 threads, 270 items, 15 pairs, rag
  3-D blocked    (65,2,3)3  3<0,L>256 0<2,S>4/T16!lin 4<3,S>8/T16!lin      (130,3,5)2 3<1,L>512 0<3,S>8/T16!lin 4<0,L>16/T16!lin rag
                 (70,5,9)3  3<0,L>256 0<0,L>16/T16!lin 4<1,L>32/T16 rag    (66,9,17)2 3<0,L>256 0<1,L>32/T16   4<2,L>64/T16 rag
                 (65,17,2)3 3<0,L>256 0<2,L>64/T16    4<2,S>4/T16!lin rag  (70,40,3)2 3<0,L>256 0<3,L>128/T16  4<3,S>8/T16!lin rag
                 (65,130,2)1 3<0,L>256 0<1,L>512/T16  4<2,S>4/T16!lin rag  (65,300,2)2 3<0,L>256 0<2,L>1024/T8 4<2,S>4/T16!lin* rag
                 (65,3,40)2 3<0,L>256 0<3,S>8/T16!lin 4<3,L>128/T16 rag    (65,2,130)1 3<0,L>256 0<2,S>4/T16!lin 4<1,L>512/T16 rag
                 (130,40,3)67 3<1,L>512 0<3,L>128/T16* 4<3,S>8/T16!lin* 34 pairs

Largest max|Y - Y_ref| / max|Y_ref| observed on the MI355X: 1.92e-15, at (2049, 9) with l = 59 (the host FFT's largest:
3.8e-16); every case passed and the natural-layout run was bit-identical.  profiles/fft_pass_kernels_errors.json (written
by a run of this file with GSI_FFT_PASS_RECORD=<path>) holds both ratios and the launches per case.

That the cases marked * do loop was checked once on the device when this file was written: a build of fft_cov.hip that
adds 1 to one prefetched element of every item after a workgroup's first failed exactly those six cases
((70,300)19, (300,33)131, (2049,9)59, (9,130,9)29, (65,300,2)2, (130,40,3)67) and passed the other 52.

Out of reach from the Python API: which instantiation actually ran (no C ABI hook is added for it) -- the model is a
reading of the launcher, checked on the CPU against the recorded kernel names only.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fft_pass_model as fm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BAR = 1e-12
RECORD_ENV = "GSI_FFT_PASS_RECORD"

_inputs = {}       # case -> (tab, X, Y_ref): computed once, never modified
_default_run = {}  # case -> (Y, Yt) of this process (every layout knob at its default)
_record = {}


def inputs(case):
    if case not in _inputs:
        Ns, l = case
        tab, X = fm.int_table(Ns), fm.int_panel(Ns, l)
        Yref = fm.exact_reference(tab, X)
        for a in (tab, X, Yref):
            a.setflags(write=False)
        _inputs[case] = (tab, X, Yref)
    return _inputs[case]


def products(gsi, ctx, case):
    """(A X, A' X) through one plan."""
    tab, X, _ = inputs(case)
    op = gsi.fft_gridcov_operator(ctx, case[0], table=tab)
    try:
        assert op.shape == (X.shape[0], X.shape[0])
        return op.matmul(X), op.rmatmul_t(X)
    finally:
        op.close()


def ratio(Y, Yref):
    return float(np.abs(Y - Yref).max() / np.abs(Yref).max())


def launch_text(p):
    return ("%s Ma=%d T=%d threads=%d lb=%d kind=%d s_lin=%s wpl=%d ragged=%s off=%s nb=%d col0=%d nitems=%d lds=%d bound=%d%s"
            % (fm.inst_name(p["inst"])[len("gsi::hipk::"):], p["Ma"], p["T"], p["threads"], p["lb"], p["kind"], p["s_lin"],
               p["wpl"], p["ragged"], p["off_form"], p["nb"], p["col0"], p["nitems"], p["shmem"], p["bound"],
               " looping" if p["looping"] else ""))


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()
    path = os.environ.get(RECORD_ENV)
    if path and _record:
        cases = [_record[fm.case_id(c)] for c in fm.CASES if fm.case_id(c) in _record]
        out = {"bar": BAR, "largest_device_ratio": max(c["device_ratio"] for c in cases),
               "largest_host_fft_ratio": max(c["host_fft_ratio"] for c in cases), "cases": cases}
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


@pytest.mark.parametrize("case", fm.CASES, ids=fm.case_id)
def test_pass_kernels_against_the_exact_product(gsi, ctx, case):
    tab, X, Yref = inputs(case)
    assert np.abs(Yref).max() > 0
    Y, Yt = products(gsi, ctx, case)
    if case in fm.BLOCKED_CASES:
        _default_run[case] = (Y, Yt)
    r, rt = ratio(Y, Yref), ratio(Yt, Yref)
    print(f"{fm.case_id(case)} max|Y - Yref| / max|Yref| = {r:.2e} (A X), {rt:.2e} (A' X)")
    if os.environ.get(RECORD_ENV):
        _record[fm.case_id(case)] = {"Ns": list(case[0]), "l": case[1], "launches": [launch_text(p) for p in fm.passes(*case)],
                                     "device_ratio": max(r, rt), "host_fft_ratio": ratio(fm.host_fft_product(tab, X), Yref)}
    assert r <= BAR, (case, r)
    assert rt <= BAR, (case, rt)


# ---- the natural layout on the grids that are blocked by default (GSI_FFT_TB is read once per process: one child) ----------
def child_main(path):
    """Runs in a child process: A X and A' X of every blocked case, saved for the parent to compare."""
    import gsi_amd as gsi
    ctx = gsi.default_context()
    out = {}
    for case in fm.BLOCKED_CASES:
        Y, Yt = products(gsi, ctx, case)
        out[fm.case_id(case)], out[fm.case_id(case) + "-t"] = Y, Yt
    np.savez(path, **out)
    print("layout-ok %d" % len(fm.BLOCKED_CASES), flush=True)


CHILD = ("import sys\n"
         "sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
         "import test_fft_pass_kernels_gpu as t\n"
         "t.child_main(sys.argv[3])\n")


def test_natural_layout_on_the_blocked_grids_is_bit_identical(gsi, ctx, tmp_path):
    """GSI_FFT_TB=0 keeps the intermediate array in its natural layout.  The layout decides where a value is stored between
    the passes and how many lines a strided tile holds, never the arithmetic of a line (the same twiddles, butterflies and
    spectrum entries in the same order), so the results must be the same bits as the default run's -- and meet the bar."""
    path = str(tmp_path / "natural.npz")
    env = dict(os.environ)
    env["GSI_FFT_TB"] = "0"
    env.pop(RECORD_ENV, None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, HERE, path], capture_output=True, text=True, timeout=300, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    assert r.stdout.count("layout-ok %d" % len(fm.BLOCKED_CASES)) == 1, r.stdout[-2000:]
    with np.load(path) as f:
        got = {k: f[k] for k in f.files}
    os.remove(path)
    for case in fm.BLOCKED_CASES:
        Yref = inputs(case)[2]
        if case not in _default_run:
            _default_run[case] = products(gsi, ctx, case)
        for Yd, key in zip(_default_run[case], (fm.case_id(case), fm.case_id(case) + "-t")):
            assert ratio(got[key], Yref) <= BAR, (case, key)
            assert np.array_equal(got[key], Yd), (case, key, float(np.abs(got[key] - Yd).max()))
