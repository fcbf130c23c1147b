"""Every kernel path of the scattered-point covariance product, entry by entry: gemm_f64.hip's GEN 2 loader and all eight
pointcov_wide_kernel<NTQ, MT, RGN> instantiations (csrc/pointcov_gemm.hip), each with one K split and with several, with
short reductions (1, 2, 3, even and odd tile counts under both prefetch schedules), ragged rows and columns, 1 to 3 column
chunks, and row / reduction offsets under the "does the diagonal cross this slot" test (three rank threads, A X and A' X).

The matrix G is never stored, so an entry is read through a product with a ONE-HOT panel: column c of X is e_{k_c}.  With
one unit entry per column the MFMA chain and the sum over the split slabs add exact zeros to one value: Y[:, c] is the
generated G[:, k_c] bit for bit.  A case's one-hot products together select every reduction index.

Checks per case (tests/pointcov_model.py holds the table, the reference and the bars; test_pointcov_model.py proves on the
CPU what the table reaches and runs the same checks on the CPU reference backend):

  entries   |G - A| <= bar A per entry, bar = 16 (1 + arg + delta) 2^-53 against the long-double reference A of the unscaled
            points (derivation: pointcov_model's docstring); far-tail entries (A < 2^-1000 sigma2): finite, >= 0,
            <= 2^-999 sigma2, exactly 0 where arg > 760.  For A X and A' X, and the two agree within the same bar.
  products  X ~ N(0, 1): |Y - A X|_ij <= sum_k (K 2^-53 + bar_ik) |A_ik| |X_kj| componentwise in long double, K the full
            reduction length -- the dot-product term holds for any summation order, splits included.

nugget = 0.75 sigma2 in every case (a misplaced nugget is an O(1) entry error), eight coincident off-diagonal pairs, points
out to 800 ell (exact underflow) and half the cases at UTM-like offsets.  n = 8192, l = 320 (the chooser's own split) gets
the entry check on the 320 selected columns.

The knobs are read once per process: every group of cases runs in one child process, one after another; a child that
exits non-zero fails its test and nothing is retried.

Measured on the MI355X (profiles/pointcov_entry_errors.json, written by a run of this file with
GSI_POINTCOV_RECORD=<path>): the largest entry error is 0.107 of the bar, i.e. 1.71 units of (1 + arg + delta) 2^-53
(<5,2,2>, Gaussian, n = 17, l = 320; the plain fp64 formula on the host reaches 1.53), the largest product error 0.116 of
its bound, and A X and A' X gave the same bits in all 118 cases.

That the table sees what it claims was checked once on the device with two perturbed builds of pointcov_gemm.hip: rel0 and
rel1 exchanged in the rowC nugget comparison of the MT == 3 branch failed exactly the cases of the 96-row <NTQ,3,2> kernels
with n >= 2 (43 cases) and passed the rest; the slab of split 1 scaled by 1 + 2^-30 failed exactly the cases with more than
one split (all forced-split groups and n = 8192) and passed every one-split case.

Out of reach from the Python API: which instantiation actually ran -- the model is a reading of the launcher.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pointcov_model as pm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RECORD_ENV = "GSI_POINTCOV_RECORD"
KNOBS = ("GSI_POINTCOV_ROWS", "GSI_POINTCOV_WIDE", "GSI_POINTCOV_TALL", "GSI_GEMM_FORCE_SPLIT", "GSI_LOCAL_COMM", "GSI_SHM_COMM")

_record = {}


def _run_ranks(gsi, cases, world):
    """The cases on `world` rank threads of this process (GSI_LOCAL_COMM=1), one context each; every rank receives the whole
    result (rows gathered / partial sums reduced), which must be the same bits on all of them."""
    import threading
    import traceback
    ctx0 = gsi.Context(0)
    uid = ctx0.unique_id()
    res, errs = [dict() for _ in range(world)], []

    def run(rank):
        try:
            ctx = ctx0 if rank == 0 else gsi.Context(0)
            ctx.comm_init(world, rank, uid)
            for case in cases:
                for k, v in pm.run_case(gsi, ctx, case).items():
                    res[rank][pm.case_id(case) + "/" + k] = v
            if rank != 0:
                ctx.close()
        except Exception:
            errs.append((rank, traceback.format_exc()))

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    if errs:
        print(errs[0][1])
        raise SystemExit(1)
    for r in range(1, world):
        assert res[r].keys() == res[0].keys()
        for k in res[0]:
            assert np.array_equal(res[r][k], res[0][k]), (r, k)
    return res[0]


def child_main(group, path):
    """Runs in a child process: the products of every case of the group, saved for the parent to check."""
    import gsi_amd as gsi
    cases = pm.group_cases(group)
    world = pm.ENVS[cases[0].env].ranks
    if world == 1:
        ctx = gsi.default_context()
        out = {}
        for case in cases:
            for k, v in pm.run_case(gsi, ctx, case).items():
                out[pm.case_id(case) + "/" + k] = v
    else:
        out = _run_ranks(gsi, cases, world)
    np.savez(path, **out)
    print("pointcov-ok %d" % len(cases), flush=True)


CHILD = ("import sys\n"
         "sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
         "import test_pointcov_kernels_gpu as t\n"
         "t.child_main(sys.argv[3], sys.argv[4])\n")


@pytest.fixture(scope="module")
def record():
    yield _record
    path = os.environ.get(RECORD_ENV)
    if path and _record:
        cases = [_record[pm.case_id(c)] for c in pm.CASES if pm.case_id(c) in _record]
        out = {"bar": "16 (1 + arg + delta) 2^-53 per entry; products: sum_k (K 2^-53 + bar_ik) |A_ik| |X_kj|",
               "largest_entry_ratio": max(max(c["entries"], c["entries_t"]) for c in cases),
               "largest_mul_vs_mul_t_ratio": max(c["mul_vs_mul_t"] for c in cases),
               "largest_product_ratio": max(max(c.get("product", 0.0), c.get("product_t", 0.0)) for c in cases),
               "all_bit_identical": all(c["bit_identical"] for c in cases), "cases": cases}
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


@pytest.mark.parametrize("group", pm.GROUPS)
def test_pointcov_entries_and_products(gsi, record, tmp_path, group):
    cases = pm.group_cases(group)
    e = pm.ENVS[cases[0].env]
    assert all(c.env == cases[0].env for c in cases)
    path = str(tmp_path / "run.npz")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS and k != RECORD_ENV}
    env.update(e.vars)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, HERE, group, path], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, (group, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    assert r.stdout.count("pointcov-ok %d" % len(cases)) == 1, r.stdout[-2000:]
    with np.load(path) as f:
        got = {k: f[k] for k in f.files}
    os.remove(path)
    failures = []
    for case in cases:
        cid = pm.case_id(case)
        run = {k[len(cid) + 1:]: v for k, v in got.items() if k.startswith(cid + "/")}
        kernels = sorted({"GEN2" if m["kernel"] == pm.GEN2 else "<%d,%d,%d>x%d" % (m["kernel"] + (m["ns_eff"],))
                          for _, _, m in pm.launches(case) if m is not None})
        try:
            rec = pm.check_case(case, run)
        except AssertionError as ex:
            failures.append("%s %s: %s" % (cid, kernels, ex))
            print("FAILED", cid, kernels, ex)
            continue
        rec["kernels"] = kernels
        record[cid] = rec
        print("%s %s entries %.3f / %.3f of the bar (A X / A' X), A X vs A' X %.3f%s, products %s"
              % (cid, kernels, rec["entries"], rec["entries_t"], rec["mul_vs_mul_t"],
                 " (same bits)" if rec["bit_identical"] else "",
                 "%.3f / %.3f of the bound" % (rec["product"], rec["product_t"]) if "product" in rec else "-"))
    assert not failures, "\n".join(failures)
