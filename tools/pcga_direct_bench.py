#!/usr/bin/env python3
"""Measure pcgadirect's saddle-point solve on the device and write profiles/pcga_direct.json.

(a) For nobs in {1024, 4096, 8192}, K = 256, R = sigma^2 I: milliseconds of `gsi_pcgamat_solve` (host clock around the
    synchronised call, best of 5; the upload of b and the download of x included), its formation and factorization parts
    from the context's phase events, the factorization as nobs^3/3 flops over the 78.6 TFLOP/s fp64 MFMA peak, the host
    `pinv` step of solver="pinv" (the dense (nobs+1)^2 matrix assembled and pseudo-inverted), and a host LAPACK Cholesky
    solve of the same system beside them.  The pseudo-inverse is timed once, not five times, above nobs = 1024 (it runs for
    tens of seconds) and not at all above --pinv-max-nobs.
(b) The C5 setup of tools/pcga_forward_bench.py (n = 10^6, K = 256, nobs = 4096, a LinearForwardModel beside a DeviceBasis):
    seconds per pcgadirect iteration with solver="pinv" and solver="cholesky".

    python3 tools/pcga_direct_bench.py [--out profiles/pcga_direct.json] [--sizes 1024,4096,8192] [--no-c5] [--reps 5] [--pinv-max-nobs 4096]

A run with fewer sizes, or with --no-c5, keeps what an earlier run wrote into the same file for the parts it skips.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP64_MFMA = 78.6e12


def best_of(fn, reps, ctx):
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def one_size(gsi, ctx, nobs, K, reps, pinv_max_nobs):
    import scipy.sparse as sp
    from scipy.linalg import cho_factor, cho_solve
    rng = np.random.default_rng(nobs)
    E = rng.standard_normal((nobs, K))
    HX = rng.standard_normal(nobs)
    sigma2 = 1e-2
    b = np.concatenate([rng.standard_normal(nobs), np.zeros(1)])
    A = gsi.PCGALowRankMatrix([np.ascontiguousarray(E[:, i]) for i in range(K)], HX, sigma2 * sp.identity(nobs, format="csc"),
                              ctx=ctx)
    x, info = A.solve(b, return_info=True)                          # warm-up: code objects, workspaces
    assert info == [0, 1], info
    row = {"nobs": nobs, "K": K, "reps": reps}
    row["solve_ms"] = 1e3 * best_of(lambda: A.solve(b), reps, ctx)
    form, fact = [], []
    ctx.profile(True)
    for _ in range(reps):
        ctx.phase_reset()
        A.solve(b)
        t = ctx.phase_times()
        form.append(t["small_gemm"][0])
        fact.append(t["other"][0])
    ctx.profile(False)
    A.close()
    row["formation_ms"] = min(form)
    row["factorization_ms"] = min(fact)
    row["factorization_flops"] = nobs ** 3 / 3.0
    row["factorization_tflops"] = row["factorization_flops"] / (1e-3 * row["factorization_ms"]) / 1e12
    row["factorization_fraction_of_fp64_mfma_peak"] = row["factorization_tflops"] * 1e12 / PEAK_FP64_MFMA

    def host_cholesky():
        M = E @ E.T + sigma2 * np.eye(nobs)
        cf = cho_factor(M, lower=True)
        u, v = cho_solve(cf, HX), cho_solve(cf, b[:-1])
        beta = (HX @ v - b[-1]) / (HX @ u)
        return np.concatenate([v - beta * u, [beta]])

    def host_pinv():
        HQH = E @ E.T
        bigA = np.block([[HQH + sigma2 * np.eye(nobs), HX[:, None]], [HX[None, :], np.zeros((1, 1))]])
        return np.linalg.pinv(bigA) @ b

    xc = host_cholesky()
    row["host_lapack_cholesky_ms"] = 1e3 * best_of(host_cholesky, reps, ctx)
    row["device_vs_host_cholesky_rel_diff"] = float(np.linalg.norm(x - xc) / np.linalg.norm(xc))
    if nobs > pinv_max_nobs:                      # minutes of host SVD: not measured (it grows as nobs^3 from the sizes below)
        row["host_pinv_ms"] = None
        return row
    pinv_reps = reps if nobs <= 1024 else 1
    row["host_pinv_reps"] = pinv_reps
    xp = [None]
    row["host_pinv_ms"] = 1e3 * best_of(lambda: xp.__setitem__(0, host_pinv()), pinv_reps, ctx)
    row["device_vs_host_pinv_rel_diff"] = float(np.linalg.norm(x - xp[0]) / np.linalg.norm(xp[0]))
    row["speedup_over_host_pinv"] = row["host_pinv_ms"] / row["solve_ms"]
    return row


def c5(gsi, ctx):
    import scipy.sparse as sp
    n, Ns, K, p, q, nobs = 1000000, 256, 256, 64, 1, 4096
    op = gsi.lowrank_synthetic_operator(ctx, n, Ns, seed=3, decay=0.75)
    Om = gsi.DeviceMatrix(ctx, n, K + p).randn(9)
    Z = gsi.DeviceMatrix(ctx, n, K + p)
    gsi._lib.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, None), ctx.lib)
    Om.close()
    op.close()
    basis = gsi.DeviceBasis(Z, K)
    rng = np.random.default_rng(8)
    idx = np.arange(nobs) * (n // nobs) + 17
    xw = 1.0 + 0.1 * rng.standard_normal(n)
    sel = (np.arange(nobs + 1, dtype=np.int64), idx.astype(np.int64), np.ones(nobs), (nobs, n))
    fwd = gsi.LinearForwardModel(sel, weights=xw, ctx=ctx)
    X = np.full(n, 2.0)
    coef = rng.standard_normal(6) * 3.0
    truth = X + sum(c * basis[i] for i, c in enumerate(coef))
    noise = 1e-4
    y = (truth * xw)[idx] + noise * rng.standard_normal(nobs)
    R = noise ** 2 * sp.identity(nobs, format="csc")
    out = {"n": n, "K": K, "nobs": nobs, "iterations_timed": 1}
    sols = {}
    gsi.pcgadirect(fwd, X.copy(), X, basis, R, y, maxiters=1, solver="cholesky")                 # warm-up
    for solver, reps in (("cholesky", 3), ("pinv", 1)):
        t = best_of(lambda: sols.__setitem__(solver, gsi.pcgadirect(fwd, X.copy(), X, basis, R, y, maxiters=1, solver=solver)),
                    reps, ctx)
        out[f"seconds_per_iteration_{solver}"] = t
        out[f"reps_{solver}"] = reps
        if solver == "cholesky":
            out["fallbacks_cholesky"] = int(gsi.pcgadirect.last_fallbacks)
    out["cholesky_vs_pinv_rel_diff"] = float(np.linalg.norm(sols["cholesky"] - sols["pinv"]) / np.linalg.norm(sols["pinv"]))
    out["rel_error_vs_truth_cholesky"] = float(np.linalg.norm(sols["cholesky"] - truth) / np.linalg.norm(truth - X))
    out["rel_error_vs_truth_pinv"] = float(np.linalg.norm(sols["pinv"] - truth) / np.linalg.norm(truth - X))
    out["cholesky_not_slower_than_pinv"] = bool(out["seconds_per_iteration_cholesky"] <= out["seconds_per_iteration_pinv"])
    fwd.close()
    basis.close()
    Z.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcga_direct.json"))
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pinv-max-nobs", type=int, default=4096, help="largest nobs at which the host pinv step is timed")
    args = ap.parse_args()
    import gsi_amd as gsi
    ctx = gsi.default_context()
    os.environ.pop("GSI_SADDLE_HOST", None)
    res = {}
    if os.path.exists(args.out):
        res = json.load(open(args.out))
    res["what"] = ("tools/pcga_direct_bench.py: pcgadirect's saddle-point system by Cholesky on the device (DESIGN.md section "
                   "4.7c); host clock around synchronised calls, best of the repetitions; formation and factorization parts from "
                   "the context's phase events; one GPU")
    res["fp64_mfma_peak_tflops"] = PEAK_FP64_MFMA / 1e12
    res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", 0)) or None
    sizes = {str(r["nobs"]): r for r in res.get("sizes", [])}
    for nobs in [int(v) for v in args.sizes.split(",") if v]:
        sizes[str(nobs)] = one_size(gsi, ctx, nobs, 256, args.reps, args.pinv_max_nobs)
        print(sizes[str(nobs)], flush=True)
        res["sizes"] = [sizes[k] for k in sorted(sizes, key=int)]
        _write(args.out, res)
    if not args.no_c5:
        res["c5"] = c5(gsi, ctx)
        print(res["c5"], flush=True)
    _write(args.out, res)
    if "c5" in res and not res["c5"]["cholesky_not_slower_than_pinv"]:
        sys.exit("the cholesky iteration is slower than the pinv iteration of the same run: see " + args.out)


def _write(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
