#!/usr/bin/env python3
"""What the operator H C H' of a linear forward model costs on the device (`gsi_op_fwd_cov`: csrc/fwd_adjoint.hip, the grid
operator's passes, csrc/pcga_forward.hip), and what it is measured against.

Writes one JSON document (default profiles/fwd_cov.json).  Every time is a host clock around calls ended by a device
synchronise, the best of `reps`; every number says what it is:
  * `product`: `gsi_op_mul_dev` of the nobs x nobs operator with an nobs x b panel already in HBM, b = 64 and 320; `stage_ms`
    are the library's own event timers around the three stages of the same calls (the adjoint H' is reported as phase gemm_t,
    the grid product C as gemm_n, the forward product H as other), `bytes` what each stage moves by its shapes, `tb_s` the
    two together, beside the 6.3 TB/s of a device copy;
  * `csr_against_spread`: the adjoint with H = W, the interpolation matrix at m points stored as CSR, against the specialised
    spread of `gsi_fftrf_spread` at the same points in the same process; the index reads 12 bytes per contribution (row,
    value) where the spread reads 5 (point, corner) and recomputes the weight;
  * `composed_path`: what the adjoint replaces -- download V, scipy `H.T @ V`, upload -- as measured (nothing extrapolated);
  * `skewed`: the same rays with every ray starting in one cell (one list of at least nrays entries), and the ratio of its
    adjoint to the even one (the guide's figure for a chunked inverted-index pass under skew is 1.1-1.2 x);
  * `linear_inversion`: one inversion end to end with its iteration counts, without and with a rank-256 preconditioner.
  python3 tools/fwd_cov_bench.py [--out PATH] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gsi_amd as gsi  # noqa: E402

COPY_TB_S = 6.3


def best_ms(ctx, f, reps):
    f()
    ctx.sync()                                        # warm-up: code objects, workspaces, the lazy index
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"best": float(min(ts)), "all": ts}


def rays(Ns, nrays, nsamp, seed, one_start=False):
    """CSR of `nrays` straight rays of `nsamp` samples on the grid Ns (2-D, vec() order): a ray is the average of its samples"""
    rng = np.random.default_rng(seed)
    top = np.array(Ns, dtype=float)[:, None] - 1e-9
    a, b = rng.random((2, nrays)) * top, rng.random((2, nrays)) * top
    if one_start:
        a[:] = (0.37 * top)
    t = (np.arange(nsamp) + 0.5) / nsamp
    pts = a[:, :, None] + (b - a)[:, :, None] * t[None, None, :]
    if one_start:
        pts[:, :, 0] = a                                  # the first sample of every ray: the same cell
    cells = np.floor(pts[0]).astype(np.int64) + Ns[0] * np.floor(pts[1]).astype(np.int64)
    indptr = np.arange(nrays + 1, dtype=np.int64) * nsamp
    return indptr, cells.reshape(-1), np.full(nrays * nsamp, 1.0 / nsamp)


def time_product(ctx, op, mdl, n, b, reps):
    X = gsi.DeviceMatrix(ctx, mdl.nobs, b).randn(1)
    Y = gsi.DeviceMatrix(ctx, mdl.nobs, b)
    mul = lambda: gsi._lib.check(ctx.lib.gsi_op_mul_dev(ctx.h, op.h, 0, X.h, Y.h), ctx.lib)
    mul()
    ctx.sync()
    ctx.profile(True)
    ctx.phase_reset()
    call = best_ms(ctx, mul, reps)
    ph = ctx.phase_times()
    ctx.profile(False)
    stage = {name: ph[key][0] / (reps + 1) for name, key in (("adjoint", "gemm_t"), ("grid_product", "gemm_n"), ("forward", "other"))}
    nnz, nobs = mdl.nnz, mdl.nobs
    groups = -(-b // 8)
    by = {"adjoint": 8 * n * b + groups * (8 * (n + 1) + 12 * nnz) + 8 * nnz * b,     # stores; the index per 8 columns; V gathers
          "forward": 8 * nobs * b + -(-b // 16) * 12 * nnz + 8 * nnz * b,              # stores; the CSR per 16 columns; panel gathers
          "grid_product": 2 * 8 * n * b}                                              # the panel in and out (the passes' own traffic not counted)
    X.close(); Y.close()
    return {"columns": b, "call_ms": call, "stage_ms": stage, "bytes": by,
            "tb_s": {k: by[k] / (stage[k] * 1e-3) / 1e12 for k in stage if stage[k] > 0}, "device_copy_tb_s": COPY_TB_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fwd_cov.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    import scipy.sparse as sp
    ctx = gsi.Context(0)
    if a.small:
        Ns, nrays, nsamp, bs, reps, m, rank = (100, 100), 256, 128, (8, 32), 2, 10_000, 32
    else:
        Ns, nrays, nsamp, bs, reps, m, rank = (1000, 1000), 4096, 1024, (64, 320), 5, 1_000_000, 256
    n = int(np.prod(Ns))
    doc = {"what": " ".join(__doc__.split("\n")[0:2]), "toy_sizes": bool(a.small), "Ns": list(Ns), "rays": nrays,
           "cells_per_ray": nsamp, "grid_kernel": "exponential, ell = 20 grid spacings", "timing": f"host clock, best of {reps}",
           "one_gpu_one_run": True}
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=20.0)

    # ---- the operator, even rays
    indptr, indices, data = rays(Ns, nrays, nsamp, 0)
    mdl = gsi.LinearForwardModel((indptr, indices, data, (nrays, n)), ctx=ctx)
    op = gsi.linear_data_operator(gop, mdl)
    doc["product"] = [time_product(ctx, op, mdl, n, b, reps) for b in bs]
    doc["index"] = mdl.adjoint_info()
    print(json.dumps(doc["product"]), flush=True)

    # ---- the adjoint alone against the composed path it replaces
    b = bs[0]
    V = gsi.DeviceMatrix(ctx, nrays, b).randn(2)
    G = gsi.DeviceMatrix(ctx, n, b)
    adj = lambda: gsi._lib.check(ctx.lib.gsi_fwd_adjoint_dev(ctx.h, mdl.h, V.h, G.h), ctx.lib)
    even = best_ms(ctx, adj, reps)
    Hs = sp.csr_matrix((data, indices, indptr), shape=(nrays, n))

    def composed():
        Gh = np.asfortranarray(Hs.T @ V.to_host())
        gsi.DeviceMatrix.from_host(ctx, Gh).close()
    doc["composed_path"] = {"columns": b, "adjoint_ms": even, "download_scipy_upload_ms": best_ms(ctx, composed, reps),
                            "note": "measured at these sizes, nothing extrapolated; scipy is one host thread"}
    print(json.dumps(doc["composed_path"]), flush=True)

    # ---- skew
    ip2, ix2, dt2 = rays(Ns, nrays, nsamp, 0, one_start=True)
    skm = gsi.LinearForwardModel((ip2, ix2, dt2, (nrays, n)), ctx=ctx)
    sadj = lambda: gsi._lib.check(ctx.lib.gsi_fwd_adjoint_dev(ctx.h, skm.h, V.h, G.h), ctx.lib)
    sk = best_ms(ctx, sadj, reps)
    doc["skewed"] = {"columns": b, "adjoint_ms": sk, "index": skm.adjoint_info(), "over_even": sk["best"] / even["best"],
                     "guide_figure_for_a_chunked_inverted_index_pass": "1.1-1.2 x"}
    print(json.dumps(doc["skewed"]), flush=True)
    skm.close(); V.close(); G.close()

    # ---- H = W as CSR against the specialised spread
    P = np.asfortranarray(np.random.default_rng(5).random((2, m)))
    box = np.array([0.0, 0.0, 1.0, 1.0])
    t = P * (np.array(Ns, dtype=float)[:, None] - 1.0)
    fl = np.minimum(np.floor(t), np.array(Ns, dtype=float)[:, None] - 2.0)
    f = t - fl
    base = fl[0].astype(np.int64) + Ns[0] * fl[1].astype(np.int64)
    idx = np.stack([base, base + 1, base + Ns[0], base + Ns[0] + 1], axis=1).reshape(-1)
    wts = np.stack([(1 - f[0]) * (1 - f[1]), f[0] * (1 - f[1]), (1 - f[0]) * f[1], f[0] * f[1]], axis=1).reshape(-1)
    wm = gsi.LinearForwardModel((np.arange(m + 1, dtype=np.int64) * 4, idx, wts, (m, n)), ctx=ctx)
    Vm = gsi.DeviceMatrix(ctx, m, b).randn(3)
    Gm = gsi.DeviceMatrix(ctx, n, b)
    arr = (gsi._lib.c_i64 * 2)(*Ns)
    csr = best_ms(ctx, lambda: gsi._lib.check(ctx.lib.gsi_fwd_adjoint_dev(ctx.h, wm.h, Vm.h, Gm.h), ctx.lib), reps)
    G1 = Gm.to_host()[:, 0].copy()
    spread = best_ms(ctx, lambda: gsi._lib.check(ctx.lib.gsi_fftrf_spread(ctx.h, Gm.h, Vm.h, 2, arr, gsi._lib.dptr(P), m,
                                                                          gsi._lib.dptr(box), 0), ctx.lib), reps)
    G2 = Gm.to_host()[:, 0]
    doc["csr_against_spread"] = {"points": m, "columns": b, "csr_adjoint_ms": csr, "spread_ms": spread,
                                 "csr_over_spread": csr["best"] / spread["best"],
                                 "agree_max_rel": float(np.abs(G1 - G2).max() / np.abs(G2).max()),
                                 "index_bytes_per_contribution": {"csr": 12, "spread": 5},
                                 "note": "gsi_fftrf_spread builds and uploads its points plan inside every call; the CSR index is "
                                         "resident.  Per 8 columns the CSR pass reads 12 bytes per contribution, the spread 5 plus "
                                         "the fractions it recomputes the weights from"}
    print(json.dumps(doc["csr_against_spread"]), flush=True)
    wm.close(); Vm.close(); Gm.close()

    # ---- one inversion end to end
    rng = np.random.default_rng(7)
    y = rng.standard_normal(nrays)
    inv = {}
    for name in ("plain", f"rank_{rank}"):
        pc = gsi.lowrank_preconditioner(op, rank=rank, diag=1e-2, seed=1) if name != "plain" else None
        ctx.sync()
        t0 = time.perf_counter()
        _, _, _, rep = gsi.linear_inversion(gop, mdl, y, 1e-2, drift_grid=np.ones((n, 1)), precond=pc, tol=1e-8, return_info=True)
        ctx.sync()
        inv[name] = {"call_ms": 1e3 * (time.perf_counter() - t0), "iterations": [int(v) for v in rep["iters"]],
                     "products": rep["products"], "path": rep["path"]}
        if pc is not None:
            pc.close()
    doc["linear_inversion"] = dict(inv, noise=1e-2, tol=1e-8, drift="constant", note="the preconditioner's build is not in call_ms")
    print(json.dumps(doc["linear_inversion"]), flush=True)
    op.close(); mdl.close(); gop.close()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
