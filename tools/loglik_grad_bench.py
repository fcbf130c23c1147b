#!/usr/bin/env python3
"""What the gradient of the Gaussian log-likelihood costs on the device beside the traced solve it rides on
(`log_likelihood_grad`, `gsi_op_bilinear_terms`: csrc/bilinear_terms.hip, the derivative operators of
csrc/fft_gridcov_plan.hip).

Writes one JSON document (default profiles/loglik_grad.json).  One process; medians of 3 after a warm-up; a host clock around
calls ended by a device synchronise.  Every number says what it is:
  * `gradient`: the universal-kriging case of tools/op_logdet_bench.py -- `fft_operator_at` of a 1000 x 1000 exponential grid
    (ell = 100 spacings) at 10^5 random points, noise 0.01, drift [1, x, y], tol = 1e-8, 16 probes, preconditioned at rank 256
    by the pivoted Cholesky of the point covariance -- with the parameters log sigma2, log ell and log noise:
      `traced_solve_ms`          `gsi_op_solve_trace` on the 20 resident columns [y, G, Z]
      `precond_apply_ms`         W_z = P^-1 Z (`gsi_precond_apply`, 16 columns)
      `terms_ms`                 per parameter: one `gsi_op_bilinear_terms` call (R formed, dM R, the reduction, 32 numbers back)
      `product_ms`               per parameter: the derivative operator's product on the same 20 columns alone
      `reduction_ms`             `gsi_mat_bilinear` on the 10^5 x 20 panels alone (L, Y, R and dd), and its bytes and TB/s
      `gradient_on_top_ms`       precond_apply + the three terms calls; `gradient_over_solve` divides it by the traced solve
      `log_likelihood_ms`, `log_likelihood_grad_ms`: the whole Python calls (operators already made)
  * `reduction_1e6x64`: `gsi_mat_bilinear` alone on 10^6 x 64 panels, g = 4: with dd and R (three panels read) and without (two),
    bytes, ms and TB/s, beside `device_copy_tbs` = a device-to-device copy of one such panel measured here (read + write).
  * `operator_creation`: `fft_operator_at` with the points (host planner, inverted index, upload) and with `like=` (shared
    plan), the grid operator's creation beside them.
  * `fit`: one `fit_covariance` run end to end from sigma2 = 1, ell = 50 on data drawn at sigma2 = 2, ell = 100 (a field of
    `gridcov_sampler` read at the points, plus noise), wrt log sigma2 and log ell: wall time, evaluations, stop reason, trace.
Not measured: hardware counters, other ranks, other probe counts, other kernels.
  python3 tools/loglik_grad_bench.py [--out PATH] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gsi_amd as gsi  # noqa: E402

L = gsi._lib
K = gsi.Kriging


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


def gradient_case(ctx, Ns, ell, m, rank, reps, probes=16):
    import ctypes as C
    box = [0.0, 0.0, 1.0, 1.0]
    P = np.asfortranarray(np.random.default_rng(1).random((2, m)))
    fam = gsi.covariance_family(ctx, Ns, "exponential", points=P, box=box)
    prm = {"log_sigma2": 0.0, "log_ell": float(np.log(ell))}
    wrt = ("log_sigma2", "log_ell", "log_noise")
    op = fam.operator(prm)
    dops = fam.derivatives(prm, wrt)
    pop = gsi.pointcov_implicit_operator(ctx, P, kind="exponential", ell=ell / (Ns[0] - 1))
    G = np.column_stack([np.ones(m), P[0], P[1]])
    y = G @ np.array([1.0, 0.5, -0.5]) + np.random.default_rng(2).standard_normal(m)
    noise, tol = 0.01, 1e-8
    d = np.full(m, noise)
    pc = gsi.lowrank_preconditioner(pop, rank=rank, diag=noise, method="pivoted_cholesky")
    g, b = 4, 4 + probes
    out = {"points": m, "columns": b, "probes": probes, "tol": tol, "noise": noise, "rank": pc.rank, "parameters": list(wrt)}
    Zd, _ = K._probe_device(op, pc, probes, 0)
    Bd = gsi.DeviceMatrix.from_host(ctx, np.column_stack([y, G, Zd.to_host()]))
    Xd = gsi.DeviceMatrix(ctx, m, b)
    inf7 = (C.c_int64 * 7)()
    relres, iters, quad = np.zeros(b), np.zeros(b, dtype=np.int64), np.zeros(2 * b)
    dp, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def traced():
        L.check(ctx.lib.gsi_op_solve_trace(ctx.h, op.h, d.ctypes.data_as(dp), pc.h, Bd.h, Xd.h, probes, 512, tol, 20000, inf7,
                                           relres.ctypes.data_as(dp), iters.ctypes.data_as(i64p), quad.ctypes.data_as(dp)), ctx.lib)
    t_solve = timed(ctx, traced, reps)
    out["traced_solve_ms"] = med(t_solve)
    out["products_of_the_solve"] = int(inf7[0])
    Wz = [None]

    def apply():
        if Wz[0] is not None:
            Wz[0].close()
        Wz[0] = pc.apply(Zd)
    t_apply = timed(ctx, apply, reps)
    out["precond_apply_ms"] = med(t_apply)
    dn = [None, None, d]
    t_terms, t_prod = [], []
    Rd, Yd = gsi.DeviceMatrix(ctx, m, b), gsi.DeviceMatrix(ctx, m, b)
    L.check(ctx.lib.gsi_mat_copy_cols(ctx.h, Rd.h, 0, Xd.h, 0, g), ctx.lib)
    L.check(ctx.lib.gsi_mat_copy_cols(ctx.h, Rd.h, g, Wz[0].h, 0, probes), ctx.lib)
    for k in range(3):
        t_terms.append(timed(ctx, lambda: K.op_bilinear_terms(dops[k], dn[k], Xd, g, Wz[0]), reps))
        if dops[k] is not None:
            t_prod.append(timed(ctx, lambda: L.check(ctx.lib.gsi_op_mul_dev(ctx.h, dops[k].h, 0, Rd.h, Yd.h), ctx.lib), reps))
        else:
            t_prod.append([0.0])
    out["terms_ms"] = {wrt[k]: med(t_terms[k]) for k in range(3)}
    out["product_ms"] = {wrt[k]: med(t_prod[k]) for k in range(3)}
    t_red = timed(ctx, lambda: K.mat_bilinear(Xd, Yd, Rd, d, g), reps)
    nbytes = 3 * m * b * 8 + m * 8
    out["reduction_ms"] = dict(med(t_red), bytes=nbytes, tbs=nbytes / (np.median(t_red) * 1e-3) / 1e12)
    top = float(np.median(t_apply)) + sum(float(np.median(t)) for t in t_terms)
    out["gradient_on_top_ms"] = top
    out["gradient_over_solve"] = top / float(np.median(t_solve))
    res = {}
    t_ll = timed(ctx, lambda: res.update(a=gsi.log_likelihood(op, y, noise=noise, drift=G, precond=pc, probes=probes, tol=tol,
                                                              maxiter=20000)), reps)
    t_lg = timed(ctx, lambda: res.update(b=gsi.log_likelihood_grad(op, dops, y, noise=noise, dnoise=dn, drift=G, precond=pc,
                                                                   probes=probes, tol=tol, maxiter=20000, return_info=True)), reps)
    val, grad, info = res["b"]
    out["log_likelihood_ms"], out["log_likelihood_grad_ms"] = med(t_ll), med(t_lg)
    out["value"], out["value_equals_log_likelihood"] = float(val), bool(val == res["a"])
    out["grad"], out["grad_stderr"] = [float(v) for v in grad], [float(v) for v in info["grad_stderr"]]
    print(json.dumps({"gradient": out}), flush=True)
    # ---- operator creation, with and without the shared points plan
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=ell)
    made = []

    def fresh():
        made.append(gsi.fft_operator_at(ctx, gop, P, box=box))

    def shared():
        made.append(gsi.fft_operator_at(ctx, gop, like=op))
    t_fresh, t_like = timed(ctx, fresh, reps), timed(ctx, shared, reps)
    for h in made:
        h.close()
    t_grid = timed(ctx, lambda: gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=ell).close(), reps)
    t_dgrid = timed(ctx, lambda: gsi.fft_gridcov_derivative(ctx, list(Ns), "log_ell", kind="exponential", ell=ell).close(), reps)
    creation = {"fft_operator_at_points_ms": med(t_fresh), "fft_operator_at_like_ms": med(t_like),
                "fft_gridcov_operator_ms": med(t_grid), "fft_gridcov_derivative_ms": med(t_dgrid),
                "plan_bytes_per_point_not_uploaded_again": 48}
    print(json.dumps({"operator_creation": creation}), flush=True)
    gop.close()
    for h in (Rd, Yd, Wz[0], Bd, Xd, Zd):
        h.close()
    for o in dops + [op]:
        fam.release(o)
    # ---- one fit, end to end
    smp = gsi.gridcov_sampler(ctx, list(Ns), "exponential", ell=ell, sigma2=2.0)
    F = smp.fields(2, seed=7)
    Fp = gsi.FFTRF.interpolate(ctx, P, F, list(Ns), box=box)
    yf = Fp.to_host()[:, 0] + np.sqrt(noise) * np.random.default_rng(3).standard_normal(m)
    for h in (Fp, F, smp):
        h.close()
    start = {"log_sigma2": 0.0, "log_ell": float(np.log(ell / 2.0))}
    t0 = time.perf_counter()
    params, rep = gsi.fit_covariance(fam, start, yf, noise, drift=G[:, :1], wrt=("log_sigma2", "log_ell"), precond=pc,
                                     probes=probes, seed=0, tol=tol, gtol=1.0, maxiter=25, cg_maxiter=20000)
    ctx.sync()
    fit = {"wall_ms": 1e3 * (time.perf_counter() - t0), "evaluations": rep["evaluations"], "stop": rep["stop"], "gtol": 1.0,
           "start": start, "result": {k: float(v) for k, v in params.items()},
           "sigma2": float(np.exp(params["log_sigma2"])), "ell": float(np.exp(params["log_ell"])),
           "drawn_at": {"sigma2": 2.0, "ell": ell},
           "trace": [{"value": float(t["value"]), "grad": [float(v) for v in t["grad"]],
                      "stderr": [float(v) for v in t["stderr"]], "log_sigma2": float(t["params"]["log_sigma2"]),
                      "log_ell": float(t["params"]["log_ell"])} for t in rep["trace"]]}
    print(json.dumps({"fit": fit}), flush=True)
    pc.close()
    pop.close()
    fam.close()
    return out, creation, fit


def reduction_case(ctx, n, b, g, reps):
    Ld, Yd, Rd = (gsi.DeviceMatrix(ctx, n, b).randn(s) for s in (1, 2, 3))
    dd = np.random.default_rng(4).standard_normal(n)
    out = {"rows": n, "columns": b, "g": g}
    for label, R, d, panels in (("with_dd_and_R", Rd, dd, 3), ("without_dd", None, None, 2)):
        ts = timed(ctx, lambda: K.mat_bilinear(Ld, Yd, R, d, g), reps)
        nbytes = panels * n * b * 8
        out[label] = dict(med(ts), bytes=nbytes, tbs=nbytes / (np.median(ts) * 1e-3) / 1e12,
                          note="dd (n doubles) is uploaded inside the call" if d is not None else "")
    # a device copy of one panel, read + write
    ts = timed(ctx, lambda: L.check(ctx.lib.gsi_mat_copy_cols(ctx.h, Rd.h, 0, Yd.h, 0, b), ctx.lib), reps)
    out["device_copy_ms"] = med(ts)
    out["device_copy_tbs"] = 2 * n * b * 8 / (np.median(ts) * 1e-3) / 1e12
    a = K.mat_bilinear(Ld, Yd, Rd, dd, g)
    c = K.mat_bilinear(Ld, Yd, Rd, dd, g)
    out["two_calls_identical"] = bool(np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]))
    for h in (Ld, Yd, Rd):
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loglik_grad.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    ctx = gsi.Context(0)
    if a.small:
        Ns, ell, m, rank, reps, nred = (100, 100), 10.0, 2_000, 32, 2, 10_000
    else:
        Ns, ell, m, rank, reps, nred = (1000, 1000), 100.0, 100_000, 256, 3, 1_000_000
    doc = {"what": " ".join(__doc__.split("\n")[0:3]), "toy_sizes": bool(a.small), "repetitions": reps,
           "not_measured": "hardware counters, other ranks, other probe counts"}

    def save():
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    doc["reduction_1e6x64" if not a.small else "reduction_small"] = reduction_case(ctx, nred, 64, 4, reps)
    print(json.dumps(doc.get("reduction_1e6x64") or doc.get("reduction_small")), flush=True)
    save()
    doc["gradient"], doc["operator_creation"], doc["fit"] = gradient_case(ctx, Ns, ell, m, rank, reps)
    save()


if __name__ == "__main__":
    main()
