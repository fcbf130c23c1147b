#!/usr/bin/env python3
"""What an FFT covariance operator at scattered points costs on the device (`gsi_op_fft_at`: csrc/interp_adjoint.hip, the grid
operator's passes, csrc/fftrf_interp.hip), and what it is measured against.

Writes one JSON document (default profiles/fft_at.json).  Every number says what it is:
  * `product`: `gsi_op_mul_dev` of the m x m operator with an m x l panel already in HBM; `call_ms` is a host clock ended by a
    device synchronise, `stage_ms` the library's own event timers around the three stages of the same calls (profiling on:
    the spread W' is reported as phase gemm_t, the grid product C as gemm_n, the gather W as other), summed over the column
    batches of a product;
  * `spread_over_gather`: the spread against its yardstick, the gather kernel of the parent commit at the same shape in the
    same calls; no ratio is fixed in advance;
  * `skewed`: the same m with half of the points inside 1 % of the area, and the ratio of its spread to the uniform one
    (the guide's figure for a chunked inverted-index pass under skew is 1.1-1.2 x);
  * `grid_operator_alone`: `gsi_op_mul_dev` of the n x n grid operator with an n x l panel, same process;
  * `randsvd`: `gsi_randsvd_dev` with Omega drawn on the device;
  * `pointcov_implicit`: the exact O(m^2) operator at a point count it finishes in seconds, and that time scaled by
    (m / m_small)^2 -- an EXTRAPOLATION, marked as one;
  * `plan`: the host clock around `fft_operator_at` (host planner, inverted index, upload) and the device bytes it keeps.
  python3 tools/fft_at_bench.py [--out PATH] [--small]"""
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


def _mul_dev(ctx, op, X, Y):
    gsi._lib.check(ctx.lib.gsi_op_mul_dev(ctx.h, op.h, 0, X.h, Y.h), ctx.lib)


def time_product(ctx, op, X, Y, reps):
    """median host-clock ms of a product, and the library's stage timers of the same calls (ms per product)"""
    _mul_dev(ctx, op, X, Y)
    ctx.sync()                                        # warm-up: code objects, workspaces
    ctx.profile(True)
    ctx.phase_reset()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _mul_dev(ctx, op, X, Y)
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    ph = ctx.phase_times()
    ctx.profile(False)
    stage = {name: ph[key][0] / reps for name, key in (("spread", "gemm_t"), ("grid_product", "gemm_n"), ("gather", "other"))}
    return {"call_ms": {"median": float(np.median(ts)), "all": ts}, "stage_ms": stage}


def points_uniform(m, seed):
    return np.asfortranarray(np.random.default_rng(seed).random((2, m)))


def points_skewed(m, seed):
    """half of the points inside 1 % of the area (a 0.1 x 0.1 square), the rest uniform"""
    rng = np.random.default_rng(seed)
    P = rng.random((2, m))
    P[:, ::2] = 0.45 + 0.1 * rng.random((2, (m + 1) // 2))
    return np.asfortranarray(P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fft_at.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    ctx = gsi.Context(0)
    if a.small:
        Ns, m, l, reps, (K, p, q), m_pc = (100, 100), 10_000, 32, 2, (16, 16, 2), 4_000
    else:
        Ns, m, l, reps, (K, p, q), m_pc = (1000, 1000), 1_000_000, 320, 5, (256, 64, 2), 100_000
    n = int(np.prod(Ns))
    box = [0.0, 0.0, 1.0, 1.0]
    doc = {"what": " ".join(__doc__.split("\n")[0:2]), "toy_sizes": bool(a.small), "Ns": list(Ns), "points": m, "columns": l,
           "grid_kernel": "exponential, ell = 20 grid spacings"}
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=20.0)

    # ---- the plan
    ctx.sync()
    b0 = ctx.device_bytes()
    P = points_uniform(m, 0)
    t0 = time.perf_counter()
    op = gsi.fft_operator_at(ctx, gop, P, box=box)
    ctx.sync()
    doc["plan"] = {"build_ms_host_clock": 1e3 * (time.perf_counter() - t0), "resident_bytes": ctx.device_bytes() - b0,
                   "resident_bytes_per_point": (ctx.device_bytes() - b0) / m,
                   "note": "host planner + inverted index + upload; bytes: frac, base, nodeptr (8 (n + 1)), point + corner "
                           "(5 bytes per contribution, 2^d per point), the tables of the long nodes"}
    print(json.dumps(doc["plan"]), flush=True)

    # ---- a product and its stages, uniform points
    X = gsi.DeviceMatrix(ctx, m, l).randn(1)
    Y = gsi.DeviceMatrix(ctx, m, l)
    doc["product"] = time_product(ctx, op, X, Y, reps)
    st = doc["product"]["stage_ms"]
    doc["spread_over_gather"] = st["spread"] / st["gather"]
    d = len(Ns)
    doc["bytes_per_column"] = {"spread_plan_share": (5 * (1 << d) * m + 8 * (n + 1)) / 8, "spread_frac_gathers": 8 * d * (1 << d) * m / 8,
                               "spread_x_gathers": 8 * (1 << d) * m, "spread_store": 8 * n,
                               "gather_requested": 8 * (1 << d) * m, "gather_store": 8 * m,
                               "note": "as requested by the threads; the plan and the frac gathers are shared by the 8 columns "
                                       "a workgroup walks at once (their share per column is shown)"}
    print(json.dumps(doc["product"]), flush=True)

    # ---- randsvd
    Om = gsi.DeviceMatrix(ctx, m, K + p).randn(2)
    Z = gsi.DeviceMatrix(ctx, m, K + p)
    ts = []
    for _ in range(2):
        t0 = time.perf_counter()
        gsi._lib.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, None), ctx.lib)
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    doc["randsvd"] = {"K": K, "p": p, "q": q, "call_ms_first": ts[0], "call_ms": ts[1]}
    print(json.dumps(doc["randsvd"]), flush=True)
    Om.close(); Z.close()
    op.close()

    # ---- skew
    Ps = points_skewed(m, 3)
    ops = gsi.fft_operator_at(ctx, gop, Ps, box=box)
    sk = time_product(ctx, ops, X, Y, reps)
    ops.close()
    doc["skewed"] = dict(sk, points="half of the points inside 1 % of the area, the rest uniform",
                         spread_over_uniform_spread=sk["stage_ms"]["spread"] / st["spread"],
                         guide_figure_for_a_chunked_inverted_index_pass="1.1-1.2 x")
    print(json.dumps(doc["skewed"]), flush=True)
    X.close(); Y.close()

    # ---- the grid operator alone
    Xg = gsi.DeviceMatrix(ctx, n, l).randn(4)
    Yg = gsi.DeviceMatrix(ctx, n, l)
    _mul_dev(ctx, gop, Xg, Yg)
    ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _mul_dev(ctx, gop, Xg, Yg)
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    doc["grid_operator_alone"] = {"call_ms": {"median": float(np.median(ts)), "all": ts}}
    print(json.dumps(doc["grid_operator_alone"]), flush=True)
    Xg.close(); Yg.close()

    # ---- the exact O(m^2) operator at a point count it finishes in seconds
    pc = gsi.pointcov_implicit_operator(ctx, P[:, :m_pc] * (Ns[0] - 1), kind="exponential", ell=20.0)
    Xp = gsi.DeviceMatrix(ctx, m_pc, l).randn(5)
    Yp = gsi.DeviceMatrix(ctx, m_pc, l)
    _mul_dev(ctx, pc, Xp, Yp)
    ctx.sync()
    ts = []
    for _ in range(2):
        t0 = time.perf_counter()
        _mul_dev(ctx, pc, Xp, Yp)
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    scale = (m / m_pc) ** 2
    doc["pointcov_implicit"] = {"points_measured": m_pc, "call_ms": float(np.median(ts)), "scaled_by": scale,
                                "scaled_to_points": m, "scaled_call_ms": float(np.median(ts)) * scale,
                                "note": "an EXTRAPOLATION: the product is O(m^2), measured at points_measured and scaled by "
                                        "(m / points_measured)^2"}
    print(json.dumps(doc["pointcov_implicit"]), flush=True)
    Xp.close(); Yp.close(); pc.close(); gop.close()

    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
