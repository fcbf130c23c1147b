#!/usr/bin/env python3
"""What a kriging solve on the FFT covariance operators costs on the device (`gsi_op_solve_cg`: csrc/block_cg.hip around
the operator's product), and what the fused CG kernels are measured against.

Writes one JSON document (default profiles/op_solve.json).  One process; medians of 5 after a warm-up; a host clock around
calls ended by a device synchronise.  Every number says what it is:
  * `at_points` (a): `fft_operator_at` of a 1000 x 1000 exponential grid (ell = 100 spacings) at 10^6 random points, diag =
    0.01, b = 64 and 320 columns, a FIXED budget of 50 iterations (tol so small that no column stops).  `solve_ms` is the
    whole call; `product_ms` the operator product alone at the same b (`gsi_op_mul_dev`, same process);
    `cg_kernels_ms_per_iteration` = solve_ms / 50 - product_ms: the three panel passes and the two scalar kernels (and
    the polls).  `panel_bytes_per_iteration` = 11 panels of 8 n b bytes, by the shapes (what pass 1, 2 and 3 read and write
    of P, Q, X, R while every column is active; the n doubles of d are read by every column but are one cached vector), and
    the rate that follows beside the 6.3 TB/s of a device copy;
  * `composed` (b): the same solve with GSI_CG_COMPOSED=1 for 5 iterations: `vector_ms_per_iteration` = solve_ms / 5 -
    product_ms, the BLAS-1 entry points column by column with their host round trips; `fused_over_composed` is the ratio of
    the two per-iteration figures -- the measurement that must hold is that it is below 1;
  * `grid` (c): `fft_gridcov_operator` at n = 10^6 with a diagonal, b = 320, 50 iterations;
  * `poll_sweep`: GSI_CG_POLL = 1, 2, 4, 8, 16 on (a) at b = 64 with a fixed budget of 200 iterations: what the polls cost;
  * `kriging` (d): one `kriging_weights` (drift [1, x, y]) + `krige_to_grid` run end to end at 10^5 points to tol = 1e-8, with
    its iteration count.
Not measured: hardware counters (achieved HBM bytes), other column counts, other grids.
  python3 tools/op_solve_bench.py [--out PATH] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gsi_amd as gsi  # noqa: E402

COPY_TBS = 6.3          # the device-copy rate the elementwise passes are read against


def med(ts):
    return {"median": float(np.median(ts)), "all": [float(t) for t in ts]}


def timed(ctx, f, reps):
    f()
    ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def product_ms(ctx, op, b, reps):
    n = op.shape[0]
    X = gsi.DeviceMatrix(ctx, n, b).randn(3)
    Y = gsi.DeviceMatrix(ctx, n, b)
    ts = timed(ctx, lambda: gsi._lib.check(ctx.lib.gsi_op_mul_dev(ctx.h, op.h, 0, X.h, Y.h), ctx.lib), reps)
    X.close(); Y.close()
    return ts


def fixed_budget(ctx, op, B, d, iters, reps):
    """solve with a budget of `iters` iterations that no column can finish early; ms per call and the last report"""
    rep = {}

    def run():
        X, r = op.solve(B, diag=d, tol=1e-300, maxiter=iters, strict=False, return_info=True)
        X.close()
        rep.update(r)
    ts = timed(ctx, run, reps)
    assert rep["products"] == iters and (rep["iters"] == iters).all(), rep
    return ts, rep


def leg(ctx, op, b, d, iters, reps, composed=False):
    n = op.shape[0]
    B = gsi.DeviceMatrix(ctx, n, b).randn(7)
    if composed:
        os.environ["GSI_CG_COMPOSED"] = "1"
    try:
        ts, rep = fixed_budget(ctx, op, B, d, iters, reps)
    finally:
        os.environ.pop("GSI_CG_COMPOSED", None)
        B.close()
    tp = product_ms(ctx, op, b, reps)
    per_iter = float(np.median(ts)) / iters - float(np.median(tp))
    out = {"n": n, "columns": b, "iterations": iters, "path": rep["path"], "solve_ms": med(ts), "product_ms": med(tp),
           "solve_ms_per_iteration": float(np.median(ts)) / iters}
    if composed:
        out["vector_ms_per_iteration"] = per_iter
    else:
        pb = 11 * 8 * n * b
        out.update({"cg_kernels_ms_per_iteration": per_iter, "panel_bytes_per_iteration": pb,
                    "d_bytes_requested_per_iteration": 2 * 8 * n * b,
                    "panel_tb_per_s": pb / (per_iter * 1e-3) / 1e12, "device_copy_tb_per_s": COPY_TBS})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "op_solve.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    ctx = gsi.Context(0)
    if a.small:
        Ns, m, bs, reps, ell, m_k = (100, 100), 10_000, (8, 32), 2, 10.0, 2_000
    else:
        Ns, m, bs, reps, ell, m_k = (1000, 1000), 1_000_000, (64, 320), 5, 100.0, 100_000
    n = int(np.prod(Ns))
    box = [0.0, 0.0, 1.0, 1.0]
    doc = {"what": " ".join(__doc__.split("\n")[0:2]), "toy_sizes": bool(a.small), "Ns": list(Ns), "points": m,
           "grid_kernel": f"exponential, ell = {ell:g} grid spacings", "noise": 0.01, "repetitions": reps,
           "not_measured": "hardware counters (achieved HBM bytes), other column counts, other grids"}
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=ell)
    P = np.asfortranarray(np.random.default_rng(0).random((2, m)))
    op = gsi.fft_operator_at(ctx, gop, P, box=box)
    d = np.full(m, 0.01)

    # ---- (a) the fused kernels, (b) the composed path, same process, same shapes
    doc["at_points"], doc["composed"], doc["fused_over_composed"] = {}, {}, {}
    for b in bs:
        fa = leg(ctx, op, b, d, 50, reps)
        co = leg(ctx, op, b, d, 5, reps, composed=True)
        doc["at_points"][f"b={b}"] = fa
        doc["composed"][f"b={b}"] = co
        doc["fused_over_composed"][f"b={b}"] = fa["cg_kernels_ms_per_iteration"] / co["vector_ms_per_iteration"]
        print(json.dumps({"b": b, "fused": fa, "composed": co}), flush=True)

    # ---- the poll interval
    B = gsi.DeviceMatrix(ctx, m, bs[0]).randn(9)
    sweep = {}
    for poll in (1, 2, 4, 8, 16):
        os.environ["GSI_CG_POLL"] = str(poll)
        rep = {}

        def run():
            X, r = op.solve(B, diag=d, tol=1e-300, strict=False, maxiter=200, return_info=True)
            X.close()
            rep.update(r)
        ts = timed(ctx, run, reps)
        sweep[f"poll={poll}"] = {"call_ms": med(ts), "products": rep["products"], "polls": -(-rep["products"] // poll) + 1}
    os.environ.pop("GSI_CG_POLL", None)
    B.close()
    doc["poll_sweep"] = dict(sweep, columns=bs[0], iterations=200)
    print(json.dumps(doc["poll_sweep"]), flush=True)
    op.close()

    # ---- (c) the grid operator itself with a diagonal
    doc["grid"] = leg(ctx, gop, bs[1], np.full(n, 0.01), 50, reps)
    print(json.dumps(doc["grid"]), flush=True)

    # ---- (d) kriging end to end
    Pk = np.asfortranarray(np.random.default_rng(1).random((2, m_k)))
    opk = gsi.fft_operator_at(ctx, gop, Pk, box=box)
    rng = np.random.default_rng(2)
    G = np.column_stack([np.ones(m_k), Pk[0], Pk[1]])
    y = G @ np.array([1.0, 0.5, -0.5]) + rng.standard_normal(m_k)
    S, rep = opk.solve(np.column_stack([y, G]), diag=0.01, tol=1e-8, maxiter=20000, strict=False, return_info=True)   # warm-up, and the counts
    ctx.sync()
    t0 = time.perf_counter()
    xi, beta = gsi.kriging_weights(opk, y, noise=0.01, drift=G, tol=1e-8, maxiter=20000, strict=False)
    ctx.sync()
    t1 = time.perf_counter()
    gx, gy = np.meshgrid(np.linspace(0, 1, Ns[0]), np.linspace(0, 1, Ns[1]), indexing="ij")
    Dg = np.column_stack([np.ones(n), gx.reshape(-1, order="F"), gy.reshape(-1, order="F")])
    s = gsi.krige_to_grid(opk, xi, beta=beta, drift_grid=Dg)
    ctx.sync()
    t2 = time.perf_counter()
    doc["kriging"] = {"points": m_k, "columns": 4, "tol": 1e-8, "maxiter": 20000, "iterations_max": int(rep["iters"].max()),
                      "iterations_per_column": [int(v) for v in rep["iters"]], "products": rep["products"],
                      "converged_columns": rep["converged"], "relres_max": float(rep["relres"].max()),
                      "kriging_weights_ms": 1e3 * (t1 - t0), "krige_to_grid_ms": 1e3 * (t2 - t1),
                      "field_finite": bool(np.isfinite(s).all()), "drift_orthogonality": float(np.abs(G.T @ xi).max())}
    print(json.dumps(doc["kriging"]), flush=True)
    opk.close(); gop.close()

    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
