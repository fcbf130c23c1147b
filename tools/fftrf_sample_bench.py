#!/usr/bin/env python3
"""What sampling FFTRF power-law fields on the device costs (csrc/fftrf_sample.hip), and the host path it replaces.

Writes one JSON document (default profiles/fftrf_sample.json).  Every number says what it is:
  * `call_ms_per_field`: a host clock around `gsi_fftrf_fields` in seed mode, ended by a device synchronise -- the randn fill of
    phi, the passes, the statistics and the normalising write, NOT a kernel time from a trace;
  * `bytes_per_field`: computed from the shapes (below), and `gb_per_s` = those bytes over that time;
  * `getxis`: operator build (fields generated, centred, kept in HBM), randsvd with a device Omega, and the whole
    `getxis_fftrf(..., device=True)` call whose Omega is drawn on the host and uploaded;
  * `host_path`: `oracle.fftrf_powerlaw_structuredgrid` for a few fields plus `gsi_op_lowrank`'s upload of them, scaled to
    the field count -- an EXTRAPOLATION, marked as one.
  python3 tools/fftrf_sample_bench.py [--out PATH] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gsi_amd as gsi  # noqa: E402
import fftrf_model as fm  # noqa: E402


def bytes_per_field(Ns):
    """HBM bytes one field must move: phi written by the fill and read by pass 1, every pass's complex reads and writes with
    the crop behind each axis, the real field written once and read three times (two reductions, the normalising write),
    the destination written once."""
    A, L, _, _ = fm.geometry(Ns)
    mtot, n = int(np.prod(L)), int(np.prod(A))
    b = 8 * mtot * 2                                   # phi: fill + pass 1
    cur = list(L)
    for a in range(len(A)):
        last = a == len(A) - 1
        if a > 0:
            b += 16 * int(np.prod(cur))                # read the cropped array of the previous pass
        cur[a] = A[a]
        b += (8 if last else 16) * int(np.prod(cur))   # the last pass stores the real part only
    b += 8 * n * 3 + 8 * n
    return b


def time_fields(ctx, Ns, nf, reps):
    F = gsi.DeviceMatrix(ctx, int(np.prod(Ns)), nf)
    arr = (gsi._lib.C.c_int64 * len(Ns))(*Ns)

    def run(seed):
        gsi._lib.check(ctx.lib.gsi_fftrf_fields(ctx.h, F.h, len(Ns), arr, 2.0, 3.14, -3.5, None, 0, seed, 0), ctx.lib)
        ctx.sync()

    run(1)                                             # warm-up: code objects, workspace
    ts = []
    for r in range(reps):
        t0 = time.perf_counter()
        run(2 + r)
        ts.append(time.perf_counter() - t0)
    col = F.to_host()[:, :1] if nf <= 4 else None
    F.close()
    bpf = bytes_per_field(Ns)
    ms = [1e3 * t / nf for t in ts]
    return {"Ns": list(Ns), "fields": nf, "repeats": reps, "call_ms_per_field": {"median": float(np.median(ms)), "all": ms},
            "bytes_per_field": bpf, "gb_per_s": bpf / (float(np.median(ms)) * 1e-3) / 1e9,
            "launches": fm.launches(Ns)}, col


def time_getxis(ctx, Ns, nf, K, p, q):
    n = int(np.prod(Ns))
    out = {"Ns": list(Ns), "fields": nf, "rank": K, "p": p, "q": q}
    for rep in range(2):
        t0 = time.perf_counter()
        op = gsi.lowrank_fftrf_operator(ctx, Ns, 2.0, 3.14, -3.5, nf, seed=0)
        ctx.sync()
        t_op = time.perf_counter() - t0
        Om = gsi.DeviceMatrix(ctx, n, K + p).randn(5)
        Z = gsi.DeviceMatrix(ctx, n, K + p)
        ctx.sync()
        t0 = time.perf_counter()
        gsi._lib.check(ctx.lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, p, q, Z.h, None), ctx.lib)
        ctx.sync()
        t_svd = time.perf_counter() - t0
        Om.close(); Z.close(); op.close()
        out["operator_build_ms" if rep else "operator_build_ms_first"] = 1e3 * t_op
        out["randsvd_device_omega_ms" if rep else "randsvd_device_omega_ms_first"] = 1e3 * t_svd
    t0 = time.perf_counter()
    basis = gsi.getxis_fftrf(Ns, 2.0, 3.14, -3.5, nf, K, p, q, seed=0, ctx=ctx, device=True)
    ctx.sync()
    out["getxis_fftrf_total_ms_host_omega"] = 1e3 * (time.perf_counter() - t0)
    x0 = basis[0]
    out["xi0_finite"] = bool(np.isfinite(x0).all())
    return out


def time_host_path(ctx, Ns, nf_total, nf_meas):
    rng = np.random.default_rng(0)
    from oracle import oracle as orc
    t0 = time.perf_counter()
    fields = [orc.fftrf_powerlaw_structuredgrid(Ns, 2.0, 3.14, -3.5, rng).reshape(-1, order="F") for _ in range(nf_meas)]
    t_gen = time.perf_counter() - t0
    t0 = time.perf_counter()
    lr = gsi.LowRankCovMatrix(fields, ctx=ctx)
    lr._device_operator()
    ctx.sync()
    t_up = time.perf_counter() - t0
    lr.close()
    return {"Ns": list(Ns), "fields_measured": nf_meas, "host_generation_s": t_gen, "upload_and_centre_s": t_up,
            "extrapolated_to_fields": nf_total,
            "extrapolated_total_s": (t_gen + t_up) * nf_total / nf_meas,
            "note": "numpy restatement of FFTRF.jl:83-100 on this host's CPUs, one field after the other; an extrapolation"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fftrf_sample.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    ctx = gsi.Context(0)
    if a.small:
        w2, w3, gx, hp = ((100, 100), 16), ((16, 16, 16), 8), ((100, 100), 32, 8, 4, 2), ((100, 100), 32, 4)
    else:
        w2, w3, gx, hp = ((1000, 1000), 1024), ((128, 128, 128), 256), ((1000, 1000), 1024, 256, 64, 2), ((1000, 1000), 1024, 8)
    doc = {"what": __doc__.split("\n")[0], "toy_sizes": bool(a.small), "workloads": []}
    for Ns, nf in (w2, w3):
        r, _ = time_fields(ctx, Ns, nf, 3)
        print(json.dumps({k: r[k] for k in ("Ns", "fields", "call_ms_per_field", "gb_per_s")}), flush=True)
        doc["workloads"].append(r)
    ctx.release_cache()
    doc["getxis"] = time_getxis(ctx, *gx)
    print(json.dumps(doc["getxis"]), flush=True)
    ctx.release_cache()
    doc["host_path"] = time_host_path(ctx, *hp)
    print(json.dumps(doc["host_path"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
