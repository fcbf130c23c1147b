#!/usr/bin/env python3
"""What a Gaussian log-likelihood costs on the device beside the kriging solve it contains, and what the estimate is worth
(`log_likelihood`, `gsi_op_solve_trace`: the trace kernels and the quadrature of csrc/block_slq.hip).

Writes one JSON document (default profiles/op_logdet.json).  One process; medians of 3 after a warm-up; a host clock around
calls ended by a device synchronise.  Every number says what it is:
  * `likelihood`: the kriging case of tools/op_precond_bench.py -- `fft_operator_at` of a 1000 x 1000 exponential grid (ell =
    100 spacings) at 10^5 random points, noise 0.01, drift [1, x, y], tol = 1e-8 -- with 16 probes: the 20 columns [y, G, z_1
    .. z_16] in one traced solve, preconditioned at rank 256 by both `method`s of `lowrank_preconditioner` (the device
    randsvd of the FFT operator; the pivoted Cholesky of the point covariance that operator interpolates).  Per method:
      `log_likelihood_ms`      the whole Python call (sampling, the host link both ways, the traced solve, the host algebra)
      `sampling_ms`            the 16 probes alone: two `gsi_mat_randn`, `gsi_precond_sample`, the download
      `untraced_solve_ms`      `gsi_op_solve_pcg` on the same 20 resident columns: what the parent commit runs
      `traced_solve_ms`        `gsi_op_solve_trace` on them with quad_out = NULL: the same solve and the trace launches
      `trace_launches_ms`      traced - untraced, a difference of medians (`trace_launches_ms_per_product` divides it)
      `traced_with_quadrature_ms`, `quadrature_ms` = that - traced: the quadrature kernel, its upload and download
      `products`, `product_ms` (the operator product alone at 20 columns) and `operator_products_ms` = their product;
      `cg_kernels_ms` = untraced - operator_products_ms: the panel passes, the contractions and the scalar kernels
    and the value, its `logdet`, the standard error of the 16 probes and the iterations.
  * `accuracy`: `pointcov_implicit_operator` (exponential, ell = 0.1) at 2 x 10^4 random points + 0.01 I, preconditioned at
    rank 256 by the pivoted Cholesky: `logdet` with 16 probes, its standard error, and numpy's slogdet of the dense matrix
    side by side.  Recorded only: the estimate is statistical and there is no bar on it.
Not measured: hardware counters, other ranks, other probe counts.
  python3 tools/op_logdet_bench.py [--out PATH] [--small]"""
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
    X = gsi.DeviceMatrix(ctx, n, b)
    X.randn(3)
    Y = gsi.DeviceMatrix(ctx, n, b)
    ts = timed(ctx, lambda: L.check(ctx.lib.gsi_op_mul_dev(ctx.h, op.h, 0, X.h, Y.h), ctx.lib), reps)
    X.close()
    Y.close()
    return ts


def likelihood_case(ctx, Ns, ell, m, K, p, q, reps, maxiter, probes=16, qmax=512):
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=ell)
    P = np.asfortranarray(np.random.default_rng(1).random((2, m)))
    op = gsi.fft_operator_at(ctx, gop, P, box=[0.0, 0.0, 1.0, 1.0])
    pop = gsi.pointcov_implicit_operator(ctx, P, kind="exponential", ell=ell / (Ns[0] - 1))
    rng = np.random.default_rng(2)
    G = np.column_stack([np.ones(m), P[0], P[1]])
    y = G @ np.array([1.0, 0.5, -0.5]) + rng.standard_normal(m)
    noise, tol = 0.01, 1e-8
    d = np.full(m, noise)
    b = 4 + probes
    out = {"points": m, "columns": b, "probes": probes, "qmax": qmax, "tol": tol, "noise": noise, "rank": K}
    tp = float(np.median(product_ms(ctx, op, b, reps)))
    out["product_ms"] = tp
    makers = {"randsvd of the FFT operator": lambda: gsi.lowrank_preconditioner(op, rank=K, diag=noise, p=p, q=q, seed=5),
              "pivoted Cholesky of the point covariance":
                  lambda: gsi.lowrank_preconditioner(pop, rank=K, diag=noise, method="pivoted_cholesky")}
    i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    for label, make in makers.items():
        pc = make()
        res = {}
        t_ll = timed(ctx, lambda: res.update(v=gsi.log_likelihood(op, y, noise=noise, drift=G, precond=pc, probes=probes, seed=0,
                                                                  tol=tol, maxiter=maxiter, qmax=qmax, return_info=True)), reps)
        val, info = res["v"]
        t_s = timed(ctx, lambda: gsi.Kriging._probe_matrix(op, pc, probes, 0), reps)
        Bd = gsi.DeviceMatrix.from_host(ctx, np.column_stack([y, G, gsi.Kriging._probe_matrix(op, pc, probes, 0)]))
        Xd = gsi.DeviceMatrix(ctx, m, b)
        inf6, inf7 = (C.c_int64 * 6)(), (C.c_int64 * 7)()
        relres, iters, quad = np.zeros(b), np.zeros(b, dtype=np.int64), np.zeros(2 * b)

        def untraced():
            L.check(ctx.lib.gsi_op_solve_pcg(ctx.h, op.h, d.ctypes.data_as(dp), pc.h, Bd.h, Xd.h, tol, maxiter, inf6,
                                             relres.ctypes.data_as(dp), iters.ctypes.data_as(i64p)), ctx.lib)

        def traced(q_out):
            L.check(ctx.lib.gsi_op_solve_trace(ctx.h, op.h, d.ctypes.data_as(dp), pc.h, Bd.h, Xd.h, probes, qmax, tol, maxiter,
                                               inf7, relres.ctypes.data_as(dp), iters.ctypes.data_as(i64p), q_out), ctx.lib)
        t_u = timed(ctx, untraced, reps)
        t_t = timed(ctx, lambda: traced(None), reps)
        t_q = timed(ctx, lambda: traced(quad.ctypes.data_as(dp)), reps)
        products = int(inf7[0])
        assert products == int(inf6[0]), (products, int(inf6[0]))
        mu, mt, mq = float(np.median(t_u)), float(np.median(t_t)), float(np.median(t_q))
        out[label] = {"rank_reached": pc.rank, "log_likelihood": float(val), "logdet": info["logdet"], "logdet_P": info["logdet_P"],
                      "stderr_of_the_probe_mean": info["stderr"], "quadform": info["quadform"], "logdet_GMG": info["logdet_GMG"],
                      "iterations_per_column": [int(v) for v in info["iters"]], "truncated_columns": info["truncated"],
                      "products": products, "log_likelihood_ms": med(t_ll), "sampling_ms": med(t_s),
                      "untraced_solve_ms": med(t_u), "traced_solve_ms": med(t_t), "traced_with_quadrature_ms": med(t_q),
                      "trace_launches_ms": mt - mu, "trace_launches_ms_per_product": (mt - mu) / max(products, 1),
                      "quadrature_ms": mq - mt, "operator_products_ms": products * tp, "cg_kernels_ms": mu - products * tp}
        print(json.dumps({label: out[label]}), flush=True)
        for h in (Bd, Xd, pc):
            h.close()
    for h in (pop, op, gop):
        h.close()
    return out


def accuracy_case(ctx, m, K, probes=16):
    P = np.asfortranarray(np.random.default_rng(4).random((2, m)))
    ell, noise = 0.1, 0.01
    op = gsi.pointcov_implicit_operator(ctx, P, kind="exponential", ell=ell)
    pc = gsi.lowrank_preconditioner(op, rank=K, diag=noise, method="pivoted_cholesky")
    t0 = time.perf_counter()
    val, info = gsi.logdet(op, diag=noise, precond=pc, probes=probes, seed=0, tol=1e-8, return_info=True)
    t_est = 1e3 * (time.perf_counter() - t0)
    pc.close()
    op.close()
    t0 = time.perf_counter()
    M = np.empty((m, m))
    for i0 in range(0, m, 2000):                                 # exp(-|x_i - x_j| / ell) in row blocks
        dx = P[0, i0:i0 + 2000, None] - P[0][None, :]
        dy = P[1, i0:i0 + 2000, None] - P[1][None, :]
        M[i0:i0 + 2000] = np.exp(-np.sqrt(dx * dx + dy * dy) / ell)
    M[np.arange(m), np.arange(m)] += noise
    sign, ref = np.linalg.slogdet(M)
    t_ref = 1e3 * (time.perf_counter() - t0)
    return {"points": m, "kernel": f"exponential, ell = {ell:g}, + {noise:g} I", "rank": K, "probes": probes, "estimate": float(val),
            "stderr_of_the_probe_mean": info["stderr"], "numpy_slogdet": float(ref), "slogdet_sign": float(sign),
            "difference": float(val - ref), "difference_in_stderr": float((val - ref) / info["stderr"]),
            "relative_difference": float(abs(val - ref) / abs(ref)), "logdet_P": info["logdet_P"],
            "iterations_per_probe": [int(v) for v in info["iters"]], "estimate_ms_first_call": t_est,
            "dense_reference_ms_on_the_host": t_ref, "bar": "none: recorded only, the estimate is statistical"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "op_logdet.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    ctx = gsi.Context(0)
    if a.small:
        Ns, ell, m, K, p, reps, m_acc = (100, 100), 10.0, 2_000, 32, 16, 2, 1_000
    else:
        Ns, ell, m, K, p, reps, m_acc = (1000, 1000), 100.0, 100_000, 256, 64, 3, 20_000
    doc = {"what": " ".join(__doc__.split("\n")[0:2]), "toy_sizes": bool(a.small), "repetitions": reps,
           "not_measured": "hardware counters, other ranks, other probe counts"}

    def save():
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    doc["likelihood"] = likelihood_case(ctx, Ns, ell, m, K, p, 2, reps, 20000)
    save()
    doc["accuracy"] = accuracy_case(ctx, m_acc, K)
    print(json.dumps(doc["accuracy"]), flush=True)
    save()


if __name__ == "__main__":
    main()
