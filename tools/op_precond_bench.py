#!/usr/bin/env python3
"""What the low-rank-plus-diagonal preconditioner buys a kriging solve on the device, and what an iteration of the
preconditioned solver costs (`gsi_op_solve_pcg`: csrc/block_pcg.hip and the two contractions around the operator's product).

Writes one JSON document (default profiles/op_precond.json).  One process; medians of 5 after a warm-up; a host clock around
calls ended by a device synchronise.  Every number says what it is:
  * `kriging`: the case of DESIGN 4.6h "Limits" -- `fft_operator_at` of a 1000 x 1000 exponential grid (ell = 100 spacings) at
    10^5 random points, noise 0.01, the 4 columns [y, 1, x, y] of universal kriging, tol = 1e-8 -- solved by plain CG and by
    PCG with a rank-256 basis from the device randsvd (p = 64, q = 2), same process.  Per column: iterations; per run:
    operator products, `randsvd_ms` and `factor_ms` (the two parts of the setup, separately), `solve_ms`, and
    `end_to_end_ms` = randsvd + factor + solve.  Two shifts: 0 and the smallest kept singular value.  The condition that has
    to hold is `pcg_products_fewer`; `end_to_end_below_plain` is reported whatever it says.
  * `per_iteration`: 10^6 points, b = 64 and 320, K = 256 (a random basis: the cost does not depend on its quality), a FIXED
    budget of 20 iterations (tol so small that no column stops).  `iteration_ms` = solve_ms / 20; `product_ms` the operator
    product alone at the same b; `iteration_ms_K1` the same solve with K = 1; `contractions_ms` = iteration_ms -
    iteration_ms_K1 (by difference: what S = W'R and Y = W S cost at K = 256 beyond K = 1); `panel_kernels_ms` =
    iteration_ms_K1 - product_ms: the five panel passes, their scalar kernels and the K = 1 contractions, with
    `panel_bytes_per_iteration` = 16 panels of 8 n b bytes by the shapes and the rate that follows, beside plain CG's passes
    measured the same way in the same process (11 panels).
Not measured: hardware counters (achieved HBM bytes), other ranks, other grids.
  python3 tools/op_precond_bench.py [--out PATH] [--small]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gsi_amd as gsi  # noqa: E402

L = gsi._lib
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
    ts = timed(ctx, lambda: L.check(ctx.lib.gsi_op_mul_dev(ctx.h, op.h, 0, X.h, Y.h), ctx.lib), reps)
    X.close(); Y.close()
    return ts


def randsvd(ctx, op, K, p, q, seed):
    """Z (n x (K + p), resident) and the K + p singular values."""
    n = op.shape[0]
    Om = gsi.DeviceMatrix(ctx, n, K + p).randn(seed)
    Z = gsi.DeviceMatrix(ctx, n, K + p)
    S = gsi.DeviceMatrix(ctx, K + p, 1)
    try:
        L.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, S.h), ctx.lib)
        return Z, S.to_host()[:, 0]
    except Exception:
        Z.close()
        raise
    finally:
        Om.close()
        S.close()


def kriging_case(ctx, gop, m, box, K, p, q, reps, maxiter):
    P = np.asfortranarray(np.random.default_rng(1).random((2, m)))
    op = gsi.fft_operator_at(ctx, gop, P, box=box)
    rng = np.random.default_rng(2)
    G = np.column_stack([np.ones(m), P[0], P[1]])
    y = G @ np.array([1.0, 0.5, -0.5]) + rng.standard_normal(m)
    B = gsi.DeviceMatrix.from_host(ctx, np.column_stack([y, G]))
    noise, tol = 0.01, 1e-8
    out = {"points": m, "columns": 4, "tol": tol, "noise": noise, "rank": K, "oversampling": p, "power_steps": q}

    def solve(pc):
        rep = {}

        def run():
            X, r = op.solve(B, diag=noise, tol=tol, maxiter=maxiter, strict=False, return_info=True, precond=pc)
            X.close()
            rep.update(r)
        ts = timed(ctx, run, reps)
        return ts, rep

    ts, rep = solve(None)
    plain_ms = float(np.median(ts))
    out["plain"] = {"iterations_per_column": [int(v) for v in rep["iters"]], "products": rep["products"],
                    "converged_columns": rep["converged"], "solve_ms": med(ts)}
    print(json.dumps({"plain": out["plain"]}), flush=True)

    def rs():
        Zt, _ = randsvd(ctx, op, K, p, q, 5)
        Zt.close()
    t_rs = timed(ctx, rs, reps)
    Z, S = randsvd(ctx, op, K, p, q, 5)
    out["randsvd_ms"] = med(t_rs)
    out["singular_values"] = {"largest": float(S[0]), "smallest_kept": float(S[K - 1])}
    for label, shift in (("shift=0", 0.0), ("shift=smallest_kept_singular_value", float(S[K - 1]))):
        pcs = []

        def factor():
            while pcs:
                pcs.pop().close()
            pcs.append(gsi.lowrank_preconditioner(op, basis=Z, rank=K, diag=noise, shift=shift))
        t_f = timed(ctx, factor, reps)
        pc = pcs[0]
        ts, rep = solve(pc)
        pc.close()
        e2e = float(np.median(t_rs)) + float(np.median(t_f)) + float(np.median(ts))
        out[label] = {"shift": shift, "iterations_per_column": [int(v) for v in rep["iters"]], "products": rep["products"],
                      "converged_columns": rep["converged"], "path": rep["path"], "factor_ms": med(t_f), "solve_ms": med(ts),
                      "end_to_end_ms": e2e, "plain_solve_ms": plain_ms,
                      "pcg_products_fewer": bool(rep["products"] < out["plain"]["products"]),
                      "end_to_end_below_plain": bool(e2e < plain_ms)}
        print(json.dumps({label: out[label]}), flush=True)
    Z.close()
    B.close()
    op.close()
    return out


def per_iteration(ctx, op, b, K, iters, reps):
    n = op.shape[0]
    d = np.full(n, 0.01)
    B = gsi.DeviceMatrix(ctx, n, b).randn(7)

    def budget(pc):
        rep = {}

        def run():
            X, r = op.solve(B, diag=d, tol=1e-300, maxiter=iters, strict=False, return_info=True, precond=pc)
            X.close()
            rep.update(r)
        ts = timed(ctx, run, reps)
        assert rep["products"] == iters and (rep["iters"] == iters).all(), rep
        return float(np.median(ts)) / iters, rep

    Z = gsi.DeviceMatrix(ctx, n, K).randn(11)
    pcK = gsi.lowrank_preconditioner(op, basis=Z, diag=d)
    pc1 = gsi.lowrank_preconditioner(op, basis=Z, rank=1, diag=d)
    Z.close()
    plain, _ = budget(None)
    itK, rep = budget(pcK)
    it1, _ = budget(pc1)
    pcK.close(); pc1.close(); B.close()
    tp = float(np.median(product_ms(ctx, op, b, reps)))
    pb, pb_plain = 16 * 8 * n * b, 11 * 8 * n * b
    return {"n": n, "columns": b, "rank": K, "iterations": iters, "path": rep["path"], "iteration_ms": itK, "product_ms": tp,
            "iteration_ms_K1": it1, "contractions_ms": itK - it1, "w_bytes_read_per_iteration": 2 * 8 * n * K,
            "panel_kernels_ms": it1 - tp, "panel_bytes_per_iteration": pb, "panel_tb_per_s": pb / ((it1 - tp) * 1e-3) / 1e12,
            "plain_iteration_ms": plain, "plain_cg_kernels_ms": plain - tp, "plain_panel_bytes_per_iteration": pb_plain,
            "plain_panel_tb_per_s": pb_plain / ((plain - tp) * 1e-3) / 1e12, "device_copy_tb_per_s": COPY_TBS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "op_precond.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    ctx = gsi.Context(0)
    if a.small:
        Ns, m, bs, reps, ell, m_k, K, p = (100, 100), 10_000, (8, 32), 2, 10.0, 2_000, 32, 16
    else:
        Ns, m, bs, reps, ell, m_k, K, p = (1000, 1000), 1_000_000, (64, 320), 5, 100.0, 100_000, 256, 64
    box = [0.0, 0.0, 1.0, 1.0]
    doc = {"what": " ".join(__doc__.split("\n")[0:2]), "toy_sizes": bool(a.small), "Ns": list(Ns),
           "grid_kernel": f"exponential, ell = {ell:g} grid spacings", "repetitions": reps,
           "not_measured": "hardware counters (achieved HBM bytes), other ranks, other grids"}
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=ell)
    doc["kriging"] = kriging_case(ctx, gop, m_k, box, K, p, 2, reps, 20000)
    P = np.asfortranarray(np.random.default_rng(0).random((2, m)))
    op = gsi.fft_operator_at(ctx, gop, P, box=box)
    doc["per_iteration"] = {}
    for b in bs:
        doc["per_iteration"][f"b={b}"] = per_iteration(ctx, op, b, K, 20, reps)
        print(json.dumps(doc["per_iteration"][f"b={b}"]), flush=True)
    op.close(); gop.close()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
