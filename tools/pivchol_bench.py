#!/usr/bin/env python3
"""What the diagonal-pivoted Cholesky factorization (`gsi_op_pivoted_cholesky`: csrc/pivoted_chol.hip) costs on a
scattered-point covariance, beside the device randsvd it can replace as the source of a rank-K factor.

Writes one JSON document (default profiles/pivchol.json).  One process; medians of 5 after a warm-up; a host clock around
calls ended by a device synchronise.  Every number says what it is:
  * `factorization`: `pointcov_implicit_operator`, exponential, ell = 0.1 of the unit square, at 10^5 and 10^6 random points,
    K = 64 and 256: `ms` for the whole call into a resident L; `gb_by_shapes` = the bytes the step kernels move by their
    shapes (step j reads j columns of L and d, writes one column and d: 8 n (K (K - 1) / 2 + 3 K) bytes; the 32-byte point
    records are n of them per step on top: 32 n K) and the rate that follows, beside the device copy rate; `steps_ms`: the
    call at K = 32, 64, ... and the ms per step between two of them, i.e. against j; `launches_per_step`: by construction,
    the step kernel and the deciding workgroup (three more at the start); `polls`: as reported.
  * `randsvd`: `gsi_randsvd_dev` of the same operator at the same rank (p = 64, q = 2), 10^5 points, same process.  At 10^6
    it is not run: README's product time (10.9 s per product, six of them) stands for it.
  * `quality`: n = 2000, the dense spectrum from numpy: the trace of A - L L' (the factorization's own final trace), the
    nuclear norm of A - Z Z' for the randsvd factor, and the optimum, the sum of the eigenvalues behind the K-th.
  * `kriging`: the case of tools/op_precond_bench.py -- `fft_operator_at` of a 1000 x 1000 exponential grid (ell = 100
    spacings) at 10^5 random points, noise 0.01, the 4 columns of universal kriging, tol = 1e-8 -- preconditioned at rank 256
    with either basis.  The FFT operator has no entries to read: the pivoted Cholesky factors the point covariance of the
    same points and the same kernel, which that operator interpolates.  Per basis: the setup ms, iterations, solve ms and
    their sum.
Not measured: hardware counters (achieved HBM bytes), other kernels than the exponential, other ranks.
  python3 tools/pivchol_bench.py [--out PATH] [--small]"""
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
COPY_TBS = 6.3          # the device-copy rate the streaming passes are read against


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


def pivchol_into(ctx, op, K, Ld, tol=0.0):
    info = (C.c_int64 * 6)()
    err = (C.c_double * 3)()
    L.check(ctx.lib.gsi_op_pivoted_cholesky(ctx.h, op.h, K, float(tol), Ld.h, None, info, err), ctx.lib)
    return list(info), list(err)


def factorization(ctx, op, K, reps, step_grid):
    n = op.shape[0]
    Ld = gsi.DeviceMatrix(ctx, n, K)
    rep = {}

    def run(k=K):
        rep["info"], rep["err"] = pivchol_into(ctx, op, k, Ld)
    ts = timed(ctx, run, reps)
    info, err = rep["info"], rep["err"]
    assert info[0] == K and info[1] == 1 and info[2] == 1, info
    ms = float(np.median(ts))
    by = 8 * n * (K * (K - 1) // 2 + 3 * K) + 32 * n * K
    out = {"n": n, "K": K, "ms": med(ts), "rank": info[0], "path": "fused", "polls": info[4], "launches_per_step": 2,
           "launches_at_start": 3, "gb_by_shapes": by / 1e9, "tb_per_s_by_shapes": by / (ms * 1e-3) / 1e12,
           "device_copy_tb_per_s": COPY_TBS, "trace_left": err[1] / err[0]}
    if step_grid:
        ks = [k for k in step_grid if k <= K]
        tk = [float(np.median(timed(ctx, lambda k=k: run(k), reps))) for k in ks]
        out["steps_ms"] = {"K": ks, "call_ms": tk,
                           "ms_per_step_between": [(tk[i] - tk[i - 1]) / (ks[i] - ks[i - 1]) for i in range(1, len(ks))]}
    Ld.close()
    return out


def randsvd_ms(ctx, op, K, p, q, reps):
    n = op.shape[0]
    Om = gsi.DeviceMatrix(ctx, n, K + p).randn(5)
    Z = gsi.DeviceMatrix(ctx, n, K + p)
    ts = timed(ctx, lambda: L.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, None), ctx.lib), reps)
    Om.close()
    return ts, Z


def quality(ctx, n, K, p, q):
    P = np.asfortranarray(np.random.default_rng(4).random((2, n)))
    op = gsi.pointcov_implicit_operator(ctx, P, kind="exponential", ell=0.1)
    A = op.matmul(np.eye(n))
    lam = np.linalg.eigvalsh(0.5 * (A + A.T))[::-1]
    Ld, piv, rep = gsi.pivoted_cholesky(op, K, return_info=True)
    Lh = Ld.to_host()
    Ld.close()
    _, Zd = randsvd_ms(ctx, op, K, p, q, 1)
    Z = Zd.to_host()[:, :K]
    Zd.close()
    op.close()
    return {"n": n, "K": K, "trace": float(np.trace(A)), "optimum": float(lam[K:].sum()),
            "pivoted_cholesky_trace_error": float(np.trace(A - Lh @ Lh.T)), "pivoted_cholesky_final_trace": rep["trace"],
            "randsvd_nuclear_error": float(np.abs(np.linalg.eigvalsh(A - Z @ Z.T)).sum()),
            "randsvd_trace_error": float(np.trace(A - Z @ Z.T))}


def kriging(ctx, Ns, ell, m, K, p, q, reps, maxiter):
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=ell)
    P = np.asfortranarray(np.random.default_rng(1).random((2, m)))
    op = gsi.fft_operator_at(ctx, gop, P, box=[0.0, 0.0, 1.0, 1.0])
    pop = gsi.pointcov_implicit_operator(ctx, P, kind="exponential", ell=ell / (Ns[0] - 1))
    rng = np.random.default_rng(2)
    G = np.column_stack([np.ones(m), P[0], P[1]])
    y = G @ np.array([1.0, 0.5, -0.5]) + rng.standard_normal(m)
    B = gsi.DeviceMatrix.from_host(ctx, np.column_stack([y, G]))
    noise, tol = 0.01, 1e-8
    out = {"points": m, "columns": 4, "tol": tol, "noise": noise, "rank": K}

    def solve(pc):
        rep = {}

        def run():
            X, r = op.solve(B, diag=noise, tol=tol, maxiter=maxiter, strict=False, return_info=True, precond=pc)
            X.close()
            rep.update(r)
        return timed(ctx, run, reps), rep

    def setups():
        pcs = []

        def by_randsvd():
            while pcs:
                pcs.pop().close()
            pcs.append(gsi.lowrank_preconditioner(op, rank=K, diag=noise, p=p, q=q, seed=5))

        def by_pivchol():
            while pcs:
                pcs.pop().close()
            pcs.append(gsi.lowrank_preconditioner(pop, rank=K, diag=noise, method="pivoted_cholesky"))
        return pcs, {"randsvd of the FFT operator": by_randsvd, "pivoted Cholesky of the point covariance": by_pivchol}

    pcs, makers = setups()
    for label, make in makers.items():
        t_setup = timed(ctx, make, reps)
        ts, rep = solve(pcs[0])
        out[label] = {"setup_ms": med(t_setup), "iterations_per_column": [int(v) for v in rep["iters"]],
                      "products": rep["products"], "converged_columns": rep["converged"], "solve_ms": med(ts),
                      "end_to_end_ms": float(np.median(t_setup)) + float(np.median(ts))}
        print(json.dumps({label: out[label]}), flush=True)
    while pcs:
        pcs.pop().close()
    for h in (B, pop, op, gop):
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pivchol.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    ctx = gsi.Context(0)
    if a.small:
        ns, Ks, reps, n_rs, nq, Ns, ell, m_k = (10_000, 20_000), (16, 32), 2, 10_000, 500, (100, 100), 10.0, 2_000
    else:
        ns, Ks, reps, n_rs, nq, Ns, ell, m_k = (100_000, 1_000_000), (64, 256), 5, 100_000, 2000, (1000, 1000), 100.0, 100_000
    doc = {"what": " ".join(__doc__.split("\n")[0:2]), "toy_sizes": bool(a.small), "repetitions": reps,
           "kernel": "exponential, ell = 0.1, random points in the unit square",
           "not_measured": "hardware counters (achieved HBM bytes), other kernels, other ranks",
           "factorization": {}, "randsvd": {}}
    grid = [Ks[-1] * i // 8 for i in range(1, 9)]
    for n in ns:
        P = np.asfortranarray(np.random.default_rng(0).random((2, n)))
        op = gsi.pointcov_implicit_operator(ctx, P, kind="exponential", ell=0.1)
        for K in Ks:
            r = factorization(ctx, op, K, reps, grid if K == Ks[-1] else None)
            doc["factorization"][f"n={n} K={K}"] = r
            print(json.dumps({f"n={n} K={K}": r}), flush=True)
            if n == n_rs:
                ts, Z = randsvd_ms(ctx, op, K, Ks[0], 2, reps)
                Z.close()
                rs = float(np.median(ts))
                doc["randsvd"][f"n={n} K={K}"] = {"p": Ks[0], "q": 2, "ms": med(ts), "pivoted_cholesky_ms": r["ms"]["median"],
                                                  "randsvd_over_pivoted_cholesky": rs / r["ms"]["median"],
                                                  "pivoted_cholesky_is_faster": bool(r["ms"]["median"] < rs)}
                print(json.dumps({"randsvd": doc["randsvd"][f"n={n} K={K}"]}), flush=True)
        op.close()
    doc["quality"] = quality(ctx, nq, Ks[0], Ks[0], 2)
    print(json.dumps({"quality": doc["quality"]}), flush=True)
    doc["kriging"] = kriging(ctx, Ns, ell, m_k, Ks[-1], Ks[0], 2, reps, 20000)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
