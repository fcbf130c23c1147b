#!/usr/bin/env python3
"""Measure the sparse forward model resident on the device and write profiles/pcga_forward.json.

(a) The C5 setup of bench.py's `secondary_pcgalsqr_c5` (n = 10^6, K = 256, nobs = 4096, h(s) = (s .* x)[idx]) with the model
    as the host lambda and as a LinearForwardModel (a selection matrix with weights), for the fp64 and the fp32 basis: seconds
    per pcgalsqr iteration, the forward step alone (host clock around the synchronised call) and the bytes that cross PCIe.
(b) A tomography-like H -- 4096 rays of L consecutive cells, L in {1, 4, 16, 64, 256, 1024}, and whole-field averages
    (L = n; eight rows, and one) -- in both forms, the whole-field models over a range of segment limits.  The crossover between the forms and
    the default segment limit are read off this sweep and recorded.
(c) The GSI_FWD_HOST=1 path in the same process.

    python3 tools/pcga_forward_bench.py [--out profiles/pcga_forward.json] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best_of(fn, reps, ctx):
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    return min(ts)


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def rays(n, nobs, L, rng):
    """nobs rays of L consecutive cells each (block averages)."""
    L = int(L)
    starts = rng.integers(0, n - L + 1, size=nobs).astype(np.int64)
    indptr = (np.arange(nobs + 1, dtype=np.int64) * L)
    indices = (starts[:, None] + np.arange(L, dtype=np.int64)[None, :]).reshape(-1)
    data = np.full(indices.size, 1.0 / L)
    return indptr, indices, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcga_forward.json"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import scipy.sparse as sp
    import gsi_amd as gsi
    pcga_mod = sys.modules["gsi_amd.pcga"]
    ctx = gsi.default_context()
    for k in ("GSI_FWD_FORM", "GSI_FWD_SEG", "GSI_FWD_HOST"):
        os.environ.pop(k, None)

    # ---- (a) the C5 setup, as bench.py builds it
    n, Ns, K, p, q, nobs = 1000000, 256, 256, 64, 1, 4096
    op = gsi.lowrank_synthetic_operator(ctx, n, Ns, seed=3, decay=0.75)
    Om = gsi.DeviceMatrix(ctx, n, K + p).randn(9)
    Z = gsi.DeviceMatrix(ctx, n, K + p)
    gsi._lib.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, None), ctx.lib)
    Om.close()
    op.close()
    bases = {"fp64": gsi.DeviceBasis(Z, K), "fp32": gsi.DeviceBasis(Z, K, precision=32)}
    rng = np.random.default_rng(8)
    idx = np.arange(nobs) * (n // nobs) + 17
    xw = 1.0 + 0.1 * rng.standard_normal(n)
    forward = lambda sv: (sv * xw)[idx]
    sel = (np.arange(nobs + 1, dtype=np.int64), idx.astype(np.int64), np.ones(nobs), (nobs, n))
    fwd = gsi.LinearForwardModel(sel, weights=xw, ctx=ctx)
    X = np.full(n, 2.0)
    coef = rng.standard_normal(6) * 3.0
    truth = X + sum(c * bases["fp64"][i] for i, c in enumerate(coef))
    noise = 1e-4
    y = forward(truth) + noise * rng.standard_normal(nobs)
    R = noise ** 2 * sp.identity(nobs, format="csc")
    delta = pcga_mod.SQRT_EPS
    c5 = {"n": n, "K": K, "nobs": nobs, "iterations": 2,
          "pcie_bytes_per_forward_step_host_lambda": 8 * n * (K + 3) + 2 * 8 * n,
          "pcie_bytes_per_forward_step_device_model": 8 * nobs * (K + 3) + 2 * 8 * n}
    sols = {}
    for tag, basis in bases.items():
        r = {}
        for leg, model in (("host_lambda", forward), ("device_model", fwd)):
            gsi.pcgalsqr(model, X.copy(), X, basis, R, y, maxiters=1)                      # warm-up
            t = best_of(lambda: sols.__setitem__((tag, leg), gsi.pcgalsqr(model, X.copy(), X, basis, R, y, maxiters=2)), 2, ctx)
            r[f"seconds_per_iteration_{leg}"] = t / 2
            r[f"forward_step_seconds_{leg}"] = best_of(lambda: pcga_mod._iteration_head(model, basis, X, X, delta), args.reps, ctx)
        r["forward_step_form"] = gsi.LinearForwardModel.FORMS[fwd.info()[5]]
        with env(GSI_FWD_HOST=1):                                                           # (c)
            r["forward_step_seconds_GSI_FWD_HOST"] = best_of(lambda: basis.forward(fwd, X, X, delta), 2, ctx)
        r["model_vs_lambda_rel_diff"] = float(np.linalg.norm(sols[(tag, "device_model")] - sols[(tag, "host_lambda")])
                                              / np.linalg.norm(sols[(tag, "host_lambda")]))
        r["rel_error_vs_truth_device_model"] = float(np.linalg.norm(sols[(tag, "device_model")] - truth) / np.linalg.norm(truth - X))
        c5[tag] = r
    c5["fp32_vs_fp64_rel_diff_device_model"] = float(
        np.linalg.norm(sols[("fp32", "device_model")] - sols[("fp64", "device_model")]) / np.linalg.norm(sols[("fp64", "device_model")]))
    c5["fp32_basis_beats_fp64_device_model"] = bool(
        c5["fp32"]["seconds_per_iteration_device_model"] < c5["fp64"]["seconds_per_iteration_device_model"])
    c5["fp32_basis_beats_fp64_host_lambda"] = bool(
        c5["fp32"]["seconds_per_iteration_host_lambda"] < c5["fp64"]["seconds_per_iteration_host_lambda"])
    info = fwd.info()
    assert info[6] == 2 * len(bases), info            # only the GSI_FWD_HOST legs took the host path
    fwd.close()

    # ---- (b) rays of L cells, both forms; whole-field rows over segment limits
    s = truth
    sweep = []
    for L in (1, 4, 16, 64, 256, 1024):
        H = rays(n, 4096, L, rng)
        m = gsi.LinearForwardModel(H + ((4096, n),), weights=xw, ctx=ctx)
        row = {"row_length": L, "nobs": 4096, "nnz": int(H[0][-1])}
        for tag, basis in bases.items():
            for form in ("lane", "wave"):
                with env(GSI_FWD_FORM=form):
                    basis.forward(m, s, X, delta)
                    row[f"seconds_{form}_{tag}"] = best_of(lambda: basis.forward(m, s, X, delta), args.reps, ctx)
        m.close()
        sweep.append(row)
        print(row, flush=True)
    # the transfers every call pays whatever the form: s and X up, the results down (a model with one nonzero)
    m = gsi.LinearForwardModel((np.array([0, 1] + [1] * 4095), np.array([0]), np.array([1.0]), (4096, n)), ctx=ctx)
    floor = best_of(lambda: bases["fp64"].forward(m, s, X, delta), args.reps, ctx)
    m.close()
    whole = []
    for rows in (8, 1):
        Hn = (np.arange(rows + 1, dtype=np.int64) * n, np.tile(np.arange(n, dtype=np.int64), rows), np.full(rows * n, 1.0 / n),
              (rows, n))
        for limit in (256, 1024, 4096, 16384, 65536, 262144, n):
            with env(GSI_FWD_SEG=limit):
                m = gsi.LinearForwardModel(Hn, weights=xw, ctx=ctx)
            row = {"row_length": n, "nobs": rows, "segment_limit": limit, "segments": m.info()[3]}
            for form in ("lane", "wave"):
                if form == "lane" and (limit > 65536 or rows == 1):
                    continue                              # a few lanes walking 10^5 .. 10^6 nonzeros each: nothing to choose from
                with env(GSI_FWD_FORM=form):
                    bases["fp64"].forward(m, s, X, delta)
                    row[f"seconds_{form}_fp64"] = best_of(lambda: bases["fp64"].forward(m, s, X, delta), args.reps, ctx)
            m.close()
            whole.append(row)
            print(row, flush=True)
    cross = next((r["row_length"] for r in sweep if r["seconds_wave_fp64"] <= r["seconds_lane_fp64"]), None)
    # the limit that is nearest to the best of BOTH whole-field models: smallest worst-case ratio to each model's fastest time
    fastest = {rows: min(r["seconds_wave_fp64"] for r in whole if r["nobs"] == rows) for rows in (8, 1)}
    limits = sorted({r["segment_limit"] for r in whole})
    worst = {lim: max(r["seconds_wave_fp64"] / fastest[r["nobs"]] for r in whole if r["segment_limit"] == lim) for lim in limits}
    best_limit = min(limits, key=lambda lim: worst[lim])
    res = {"what": "tools/pcga_forward_bench.py: the sparse forward model resident on the device (DESIGN.md section 4.7b); host clock "
                   "around synchronised calls, best of the repetitions; every forward step includes the upload of s and X "
                   "and the download of its results",
           "c5": c5, "rays_4096": sweep, "whole_field_rows": whole, "transfer_floor_seconds": floor,
           "chosen": {"wave_from_mean_segment_length": cross, "crossover_rule": "smallest swept row length at which the wave form "
                      "is not slower than the lane form (fp64 basis)",
                      "segment_limit": best_limit,
                      "segment_limit_worst_ratio_to_fastest": {str(k): v for k, v in worst.items()},
                      "segment_limit_rule": "wave form on eight whole-field rows and on one: the limit whose worse ratio to each "
                                            "model's fastest time is smallest"}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["chosen"]))
    for b in bases.values():
        b.close()
    Z.close()


if __name__ == "__main__":
    main()
