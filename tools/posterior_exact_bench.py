#!/usr/bin/env python3
"""What the exact posterior variance of a linear inversion costs on the device (`gsi_op_posterior_variance`:
csrc/posterior_exact.hip around the operator's own products and the blocked Cholesky), at the shape of tools/fwd_cov_bench.py.

Writes one JSON document (default profiles/posterior_exact.json).  Every time is a host clock around calls ended by a device
synchronise; every number says what it is:
  * `direct`: `method="cholesky"` end to end (each run listed), with the library's event timers over the whole call: gemm_t =
    every adjoint H', gemm_n = every grid product C, other = the forward products H of the formation plus the row pass, lu =
    the factorization of the (2 nobs + p) x nobs trapezoid, small_gemm = the p-column algebra;
  * `formation`: the nobs products of the operator on unit columns timed on their own (`gsi_op_mul_dev` on identity panels of
    the batch width), with the same timers; `t_batches_derived` = the whole call's timers minus these (the grid product's
    share also holds the p columns of U and the one column of C_00);
  * `row_pass`: `gsi_mat_rowdot_acc` on one n x b panel on its own, best of `reps`: bytes by the shapes (the panel once, acc
    read and written) and TB/s beside the device-copy rate the project quotes;
  * `cg`: `method="cg"`'s per-batch work (solve of b unit columns at tol 1e-8, two prior adjoints, the row pass) timed on 2
    batches and SCALED to nobs columns -- extrapolated, labelled so -- without and with a rank-256 preconditioner;
  * `realizations`: the sample variance over 64 `condition_on_linear_data` realizations against the exact variance:
    correlation and mean ratio, recorded without a bar (it is statistical: 64 draws give about 18 % noise per cell).
  python3 tools/posterior_exact_bench.py [--out PATH] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gsi_amd as gsi  # noqa: E402
from fwd_cov_bench import COPY_TB_S, best_ms, rays  # noqa: E402

STAGES = (("adjoint", "gemm_t"), ("grid_product", "gemm_n"), ("forward_and_row_pass", "other"), ("factorization", "lu"),
          ("drift_algebra", "small_gemm"))


def phases(ctx, f):
    ctx.sync()
    ctx.profile(True)
    ctx.phase_reset()
    t0 = time.perf_counter()
    out = f()
    ctx.sync()
    ms = 1e3 * (time.perf_counter() - t0)
    ph = ctx.phase_times()
    ctx.profile(False)
    return out, ms, {name: float(ph[key][0]) for name, key in STAGES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_exact.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    ctx = gsi.Context(0)
    if a.small:
        Ns, nrays, nsamp, reps, rank, nreal = (100, 100), 256, 128, 2, 32, 16
    else:
        Ns, nrays, nsamp, reps, rank, nreal = (1000, 1000), 4096, 1024, 5, 256, 64
    n = int(np.prod(Ns))
    noise = 1e-2
    doc = {"what": " ".join(__doc__.split("\n")[0:2]), "toy_sizes": bool(a.small), "Ns": list(Ns), "rays": nrays,
           "cells_per_ray": nsamp, "grid_kernel": "exponential, ell = 20 grid spacings", "noise": noise, "drift": "constant",
           "one_gpu_one_run": True, "device_copy_tb_s": COPY_TB_S}
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=20.0)
    indptr, indices, data = rays(Ns, nrays, nsamp, 0)
    mdl = gsi.LinearForwardModel((indptr, indices, data, (nrays, n)), ctx=ctx)
    op = gsi.linear_data_operator(gop, mdl)
    X = np.ones((n, 1))

    # ---- the direct method, end to end: one plain run (it also warms every code object up), one with the timers
    ctx.sync()
    t0 = time.perf_counter()
    v, rep = gsi.posterior_variance_exact(op, noise, X, return_info=True)
    ctx.sync()
    first_ms = 1e3 * (time.perf_counter() - t0)
    (v2, rep), ms, ph = phases(ctx, lambda: gsi.posterior_variance_exact(op, noise, X, return_info=True))
    bw = rep["batch"]
    doc["direct"] = {"end_to_end_ms": [first_ms, ms], "second_run_has_the_timers_on": True, "report": rep, "timers_ms": ph,
                     "repeat_is_bitwise_equal": bool(np.array_equal(v, v2)),
                     "variance": {"min": float(v.min()), "max": float(v.max()), "mean": float(v.mean())}}
    print(json.dumps(doc["direct"]), flush=True)

    # ---- the formation alone: the operator on identity panels of the same width
    E = np.zeros((nrays, bw), order="F")
    Y = gsi.DeviceMatrix(ctx, nrays, bw)

    def formation():
        for c0 in range(0, nrays, bw):
            b = min(bw, nrays - c0)
            E[:] = 0.0
            E[np.arange(c0, c0 + b), np.arange(b)] = 1.0
            Ed = gsi.DeviceMatrix.from_host(ctx, E)
            gsi._lib.check(ctx.lib.gsi_op_mul_dev(ctx.h, op.h, 0, Ed.h, Y.h), ctx.lib)
            Ed.close()
    _, fms, fph = phases(ctx, formation)
    Y.close()
    doc["formation"] = {"ms": fms, "timers_ms": fph, "note": "the unit panels are uploaded from the host here, the library writes "
                        "them with a kernel"}
    doc["t_batches_derived"] = {k: ph[k] - fph[k] for k in ("adjoint", "grid_product", "forward_and_row_pass")}
    print(json.dumps(doc["formation"]), flush=True)

    # ---- the row pass on its own
    b = bw
    P = gsi.DeviceMatrix(ctx, n, b).randn(4)
    acc = gsi.DeviceMatrix.from_host(ctx, np.zeros((n, 1)))
    rp = best_ms(ctx, lambda: gsi.mat_rowdot_acc(P, P, acc), reps)
    by = 8 * n * b + 16 * n
    doc["row_pass"] = {"rows": n, "columns": b, "ms": rp, "bytes": by, "tb_s": by / (rp["best"] * 1e-3) / 1e12,
                       "device_copy_tb_s": COPY_TB_S, "timing": f"host clock, best of {reps}"}
    print(json.dumps(doc["row_pass"]), flush=True)
    P.close(); acc.close()

    # ---- method="cg": 2 batches timed, scaled to nobs columns
    K = gsi.Kriging
    cg = {}
    cb = min(bw, max(1, nrays // 2))                     # two whole batches also at toy sizes
    for name in ("plain", f"rank_{rank}"):
        pc = gsi.lowrank_preconditioner(op, rank=rank, diag=noise, seed=1) if name != "plain" else None
        acc = gsi.DeviceMatrix.from_host(ctx, np.zeros((n, 1)))
        ctx.sync()
        t0 = time.perf_counter()
        its, prods = [], 0
        for c0 in (0, cb):
            bb = min(cb, nrays - c0)
            Eh = np.zeros((nrays, bb), order="F")
            Eh[np.arange(c0, c0 + bb), np.arange(bb)] = 1.0
            hs = [gsi.DeviceMatrix.from_host(ctx, Eh)]
            U, srep = gsi.solve(op, hs[0], diag=noise, precond=pc, tol=1e-8, return_info=True)
            hs += [U, K._prior_adjoint_any(op, U), K._prior_adjoint_any(op, hs[0])]
            gsi.mat_rowdot_acc(hs[2], hs[3], acc)
            for h in hs:
                h.close()
            its.append(int(srep["iters"].max()))
            prods += int(srep["products"])
        ctx.sync()
        two = 1e3 * (time.perf_counter() - t0)
        acc.close()
        if pc is not None:
            pc.close()
        cols = min(2 * cb, nrays)
        cg[name] = {"two_batches_ms": two, "columns_timed": cols, "max_iterations_per_batch": its, "products": prods,
                    "EXTRAPOLATED_ms_for_all_columns": two * nrays / cols}
    doc["cg"] = dict(cg, tol=1e-8, batch=cb, note="measured on 2 batches of unit columns and scaled by nobs / columns_timed: an "
                     "extrapolation, not a measurement of the whole; the preconditioner's build is not in the time")
    print(json.dumps(doc["cg"]), flush=True)

    # ---- the sample variance of conditional realizations against the exact variance
    smp = gsi.gridcov_sampler(ctx, list(Ns), kind="exponential", ell=20.0, embed="auto")
    F = smp.fields(nreal, seed=11)
    y = np.random.default_rng(7).standard_normal(nrays)
    Fc = gsi.condition_on_linear_data(op, F, y, noise, seed=13, tol=1e-8)
    R = Fc.to_host()
    Fc.close(); F.close(); smp.close()
    # the realizations share the kriged mean only without a drift: compare with the variance without a drift
    v0 = gsi.posterior_variance_exact(op, noise)
    sv = R.var(axis=1, ddof=1)
    doc["realizations"] = {"count": nreal, "drift": "none (residual kriging of zero-mean fields)",
                           "correlation_of_sample_and_exact_variance": float(np.corrcoef(sv, v0)[0, 1]),
                           "mean_ratio_sample_over_exact": float(sv.mean() / v0.mean()),
                           "note": "statistical: recorded, no bar"}
    print(json.dumps(doc["realizations"]), flush=True)
    op.close(); mdl.close(); gop.close()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
