#!/usr/bin/env python3
"""Measure the PCGA posterior variance on the device and write profiles/pcga_posterior.json.

Shapes: C5 (n = 10^6, K = 256, nobs = 4096, diagonal R) and n = 10^6, K = 64, each with an fp64 and an fp32 basis.  Per shape
and precision, medians over --reps repetitions after one warm-up, host clock around synchronised calls:
  factor_ms            `PCGALowRankMatrix.posterior_factor()` (W, u, gamma; the download of W included)
  row_pass_ms          the kernel of `gsi_basis_quadform` with the factor's triangular W, from the context's phase events, with
                       its TB/s (n K elements read once) against 8 TB/s and TFLOP/s (n K (K + 1) flops of the triangular
                       product) against the 78.6 TFLOP/s fp64 matrix-core peak; row_pass_call_ms is the whole call (upload of
                       W, download of a, q, t)
  variance_ms          `gsi_pcga_posterior_variance` end to end (factor, row pass, 3 n doubles down, the finish on the host)
and beside them, in the same process, the two paths this replaces (fp64 basis only):
  composed device path the existing contraction into an n x K matrix on the device (`gsi_op_mul_dev` on resident operands), the
                       download of that matrix, and the row reduction in numpy -- all n rows, nothing extrapolated
  host path            the download of the basis and the products in numpy
The error ratios of the feature tests (tests/posterior_cases.py: posterior_variance against the dense saddle-point formula in
extended precision; the factor; the observed-point property; the row sums' largest error / bound over the kernel tests' edge
shapes) are measured on the same device and recorded under "variance_error_ratios", "factor_error_ratios",
"observed_points_max_v_over_r" and "row_sums_largest_error_over_bound".

    python3 tools/pcga_posterior_bench.py [--out profiles/pcga_posterior.json] [--reps 5] [--step-timeout 300]

Every (shape, precision) and the error ratios run in a child process of their own under --step-timeout; the parent never opens
the GPU and stops at the first child that fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP64_MFMA = 78.6e12
PEAK_HBM = 8.0e12
SHAPES = {"c5": dict(n=1000000, K=256, nobs=4096), "k64": dict(n=1000000, K=64, nobs=4096)}


def median_of(fn, reps, ctx):
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def one_shape(name, precision, reps):
    import gsi_amd as gsi
    os.environ.pop("GSI_POST_HOST", None)
    ctx = gsi.default_context()
    n, K, nobs = (SHAPES[name][k] for k in ("n", "K", "nobs"))
    Zm = gsi.DeviceMatrix(ctx, n, K).randn(5)
    basis = gsi.DeviceBasis(Zm, K, precision=precision)
    rng = np.random.default_rng(nobs + K)
    E = rng.standard_normal((nobs, K))
    HX = 1.0 + rng.standard_normal(nobs)
    import scipy.sparse as sp
    A = gsi.PCGALowRankMatrix([np.ascontiguousarray(E[:, i]) for i in range(K)], HX,
                              sp.diags(rng.uniform(1e-4, 2e-4, nobs), format="csc"), ctx=ctx)
    X = np.ones(n)
    row = dict(shape=name, n=n, K=K, nobs=nobs, precision=precision, reps=reps)
    W, u, gamma, info = A.posterior_factor(return_info=True)                 # warm-up
    assert info == [0, 1], info
    row["factor_ms"] = median_of(lambda: A.posterior_factor(), reps, ctx)
    a, q, t, info = basis.quadform(W, u, upper=True, return_info=True)       # warm-up
    assert info == [0, 1], info
    row["row_pass_call_ms"] = median_of(lambda: basis.quadform(W, u, upper=True), reps, ctx)
    ctx.profile(True)
    ks = []
    for _ in range(reps):
        ctx.phase_reset()
        basis.quadform(W, u, upper=True)
        ks.append(ctx.phase_times()["other"][0])
    ctx.profile(False)
    ms = statistics.median(ks)
    row["row_pass_ms"] = ms
    row["row_pass_bytes_read"] = n * K * (8 if precision == 64 else 4)
    row["row_pass_tb_per_s"] = row["row_pass_bytes_read"] / (1e-3 * ms) / 1e12
    row["row_pass_fraction_of_8_tb_per_s"] = row["row_pass_tb_per_s"] * 1e12 / PEAK_HBM
    row["row_pass_flops"] = float(n) * K * (K + 1)
    row["row_pass_tflops"] = row["row_pass_flops"] / (1e-3 * ms) / 1e12
    row["row_pass_fraction_of_fp64_mfma_peak"] = row["row_pass_tflops"] * 1e12 / PEAK_FP64_MFMA
    var = np.empty(n)
    dp = gsi._lib.dptr

    def variance():
        gsi._lib.check(ctx.lib.gsi_pcga_posterior_variance(ctx.h, basis.h, A.h, dp(X), None, dp(var), None), ctx.lib)

    variance()
    row["variance_ms"] = median_of(variance, reps, ctx)
    d = t - X
    row["variance_vs_parts_max_rel_diff"] = float(np.abs(var - (a + d * d / gamma)).max() / np.abs(var).max())
    if precision == 64:
        # the host path: the basis over the host link, then numpy
        Zh = [None]
        row["host_path_download_ms"] = median_of(lambda: Zh.__setitem__(0, Zm.to_host()), 1, ctx)
        Zh = Zh[0]
        out = [None]

        def host_products():
            P = Zh @ W
            dd = Zh @ u - X
            out[0] = (P * P).sum(axis=1) + dd * dd / gamma

        row["host_path_numpy_ms"] = median_of(host_products, 1, ctx)
        row["host_path_ms"] = row["host_path_download_ms"] + row["host_path_numpy_ms"]
        row["host_path_threads"] = int(os.environ.get("OMP_NUM_THREADS", 0)) or None
        row["device_vs_host_path_max_rel_diff"] = float(np.abs(var - out[0]).max() / np.abs(out[0]).max())
        # the composed device path: the contraction into an n x K matrix on resident operands, its download, numpy
        op = gsi.dense_operator(ctx, Zh)
        Wd = gsi.DeviceMatrix.from_host(ctx, W)
        Y = gsi.DeviceMatrix(ctx, n, K)

        def product():
            gsi._lib.check(ctx.lib.gsi_op_mul_dev(ctx.h, op.h, 0, Wd.h, Y.h), ctx.lib)

        product()
        row["composed_product_ms"] = median_of(product, reps, ctx)
        Yh = [None]
        row["composed_download_ms"] = median_of(lambda: Yh.__setitem__(0, Y.to_host()), 1, ctx)
        row["composed_numpy_reduction_ms"] = median_of(lambda: out.__setitem__(0, (Yh[0] * Yh[0]).sum(axis=1)), 1, ctx)
        row["composed_path_ms"] = row["composed_product_ms"] + row["composed_download_ms"] + row["composed_numpy_reduction_ms"]
        row["composed_path_rows_measured"] = n
        row["composed_path_extra_device_bytes"] = n * K * 8
        row["composed_vs_row_pass_a_max_rel_diff"] = float(np.abs(out[0] - a).max() / np.abs(a).max())
        row["row_pass_faster_than_composed_product"] = bool(row["row_pass_ms"] < row["composed_product_ms"])
    return row


def error_ratios():
    import gsi_amd as gsi
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import posterior_cases as pc
    os.environ.pop("GSI_POST_HOST", None)
    ctx = gsi.default_context()
    out = []
    for name in pc.FEATURE_CASES:
        for precision in (64, 32):
            for with_prior in (False, True):
                r = pc.check_variance(gsi, ctx, name, precision, with_prior, 1)
                out.append(dict(case=name, precision=precision, prior_variance=with_prior, max_err_over_max_v=r,
                                bar=pc.VARIANCE_BAR))
    res = {"variance_error_ratios": out, "factor_error_ratios": [], "observed_points_max_v_over_r": {}}
    for name in pc.FEATURE_CASES:
        r = pc.check_factor(gsi, ctx, name, 1)
        res["factor_error_ratios"].append(dict(case=name, wnw_minus_identity_max=r[0], u_rel=r[1], gamma_rel=r[2]))
    for precision in (64, 32):
        res["observed_points_max_v_over_r"][f"fp{precision}"] = pc.check_observed_points(gsi, ctx, precision, 1)
    worst = 0.0                                     # the kernel tests' cases: largest error / bound over every edge shape
    for precision in (64, 32):
        for K in pc.K_LIST:
            for n in pc.N_LIST:
                Z, _ = pc.kernel_inputs(n, K, False)
                basis, Zs = pc.make_basis(gsi, ctx, Z, precision)
                worst = max(worst, pc.check_kernel_case(basis, Zs, False, (n, K, precision), 1))
                pc.close_basis(basis)
    res["row_sums_largest_error_over_bound"] = worst
    return res


def _write(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcga_posterior.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--child", default=None, help="internal: one step, its result as a JSON line on stdout")
    args = ap.parse_args()
    if args.child:
        if args.child == "errors":
            res = error_ratios()
        else:
            name, precision = args.child.split(":")
            res = one_shape(name, int(precision), args.reps)
        print("RESULT " + json.dumps(res), flush=True)
        return
    res = {"what": ("tools/pcga_posterior_bench.py: the posterior variance from the resident basis (DESIGN.md section 4.7d); "
                    "medians, host clock around synchronised calls, the row pass from the context's phase events; one GPU"),
           "fp64_mfma_peak_tflops": PEAK_FP64_MFMA / 1e12, "hbm_peak_tb_per_s": PEAK_HBM / 1e12, "shapes": []}
    steps = [f"{name}:{p}" for name in SHAPES for p in (64, 32)] + ["errors"]
    for step in steps:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(args.reps)],
                           capture_output=True, text=True, timeout=args.step_timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.exit(f"step {step} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        val = json.loads(line[-1][7:])
        print(step, val, flush=True)
        if step == "errors":
            res.update(val)
        else:
            res["shapes"].append(val)
        _write(args.out, res)


if __name__ == "__main__":
    main()
