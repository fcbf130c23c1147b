#!/usr/bin/env python3
"""What FFTRF fields at scattered points cost on the device (csrc/fftrf_interp.hip behind csrc/fftrf_sample.hip), and the path
they replace.

Writes one JSON document (default profiles/fftrf_unstructured.json).  Every number says what it is:
  * `fields_at.call_ms_per_field`: a host clock around `gsi_fftrf_fields_at` in seed mode, ended by a device synchronise --
    the plan's upload, the randn fill of phi, the passes, the statistics, the normalising write into the workspace and the
    interpolation at the m points; `fields.call_ms_per_field`: the same clock around `gsi_fftrf_fields` in the same run;
  * `interpolate_only_ms_per_field`: the same clock around `gsi_fftrf_interpolate` of fields already in HBM;
  * `bytes_per_field`: computed from the shapes (below);
  * `replaced_path`: what a mesh user did before: `gsi_fftrf_fields`, download, the numpy restatement of FFTRF.interpolate
    (tests/fftrf_interp_model.py) on one core, upload -- measured for a few fields and scaled to the field count: an
    EXTRAPOLATION, marked as one;
  * `getxis`: the whole `getxis_fftrf(points=..., device=True)` call, Omega drawn on the host and uploaded.
  python3 tools/fftrf_unstructured_bench.py [--out PATH] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gsi_amd as gsi  # noqa: E402
import fftrf_interp_model as im  # noqa: E402
from fftrf_sample_bench import bytes_per_field as sampler_bytes_per_field  # noqa: E402

ARGS = (2.0, 3.14, -3.5)


def interp_bytes_per_field(Ns, m):
    """What the interpolation of ONE field moves: the gathers as requested (2^d values per point; the field itself is 8 n
    bytes and is served from cache where points share cells), the stores, and the plan, read once per thread and shared by
    the fields a workgroup walks (here: all of a batch, so its share per field is small and left out)."""
    d, n = len(Ns), int(np.prod(Ns))
    return {"gather_requested": 8 * (1 << d) * m, "field_footprint": 8 * n, "store": 8 * m,
            "plan_once_per_batch": (4 + 8 * d) * m}


def _median_ms(ts, nf):
    ms = [1e3 * t / nf for t in ts]
    return {"median": float(np.median(ms)), "all": ms}


def time_calls(ctx, Ns, P, nf, reps):
    n, m = int(np.prod(Ns)), P.shape[1]
    arr = (gsi._lib.C.c_int64 * len(Ns))(*Ns)
    pp = gsi._lib.dptr(P)
    F = gsi.DeviceMatrix(ctx, n, nf)
    G = gsi.DeviceMatrix(ctx, m, nf)
    G2 = gsi.DeviceMatrix(ctx, m, nf)

    def fields(seed):
        gsi._lib.check(ctx.lib.gsi_fftrf_fields(ctx.h, F.h, len(Ns), arr, *ARGS, None, 0, seed, 0), ctx.lib)
        ctx.sync()

    def fields_at(seed):
        gsi._lib.check(ctx.lib.gsi_fftrf_fields_at(ctx.h, G.h, len(Ns), arr, *ARGS, None, 0, seed, 0, pp, m, None, 0), ctx.lib)
        ctx.sync()

    def interp_only(_):
        gsi._lib.check(ctx.lib.gsi_fftrf_interpolate(ctx.h, G2.h, F.h, len(Ns), arr, pp, m, None, 0), ctx.lib)
        ctx.sync()

    fields(1); fields_at(1); interp_only(1)            # warm-up: code objects, workspace
    t = {"fields": [], "fields_at": [], "interp": []}
    for r in range(reps):                              # alternated: the three see the same machine
        for name, fn in (("fields", fields), ("fields_at", fields_at), ("interp", interp_only)):
            t0 = time.perf_counter()
            fn(2 + r)
            t[name].append(time.perf_counter() - t0)
    # the last repeat left the same seed in F and G: the one-step result equals the two-step one
    same = bool(np.array_equal(G.to_host()[:, :2], G2.to_host()[:, :2])) if nf >= 2 else None
    F.close(); G.close(); G2.close()
    sb = sampler_bytes_per_field(Ns)
    out = {"Ns": list(Ns), "points": m, "numfields": nf, "repeats": reps,
           "fields": {"call_ms_per_field": _median_ms(t["fields"], nf), "bytes_per_field": sb},
           "fields_at": {"call_ms_per_field": _median_ms(t["fields_at"], nf),
                         "bytes_per_field": {"sampler_with_the_normalised_field_written_to_the_workspace": sb,
                                             "interpolation": interp_bytes_per_field(Ns, m)}},
           "interpolate_only_ms_per_field": _median_ms(t["interp"], nf),
           "one_step_equals_two_step_first_columns": same}
    out["fields_at_minus_fields_ms_per_field"] = (out["fields_at"]["call_ms_per_field"]["median"]
                                                  - out["fields"]["call_ms_per_field"]["median"])
    return out


def time_replaced_path(ctx, Ns, P, nf_total, nf_meas):
    n = int(np.prod(Ns))
    t0 = time.perf_counter()
    F = gsi.FFTRF.powerlaw_fields(ctx, Ns, *ARGS, nf_meas, seed=2)
    ctx.sync()
    t_gen = time.perf_counter() - t0
    t0 = time.perf_counter()
    H = F.to_host()
    t_down = time.perf_counter() - t0
    F.close()
    t0 = time.perf_counter()
    base, frac = im.plan(P, Ns)
    t_plan = time.perf_counter() - t0
    t0 = time.perf_counter()
    V = im.interp(H, Ns, base, frac)
    t_interp = time.perf_counter() - t0
    t0 = time.perf_counter()
    D = gsi.DeviceMatrix.from_host(ctx, V)
    ctx.sync()
    t_up = time.perf_counter() - t0
    D.close()
    per_field = (t_gen + t_down + t_interp + t_up) / nf_meas
    return {"Ns": list(Ns), "points": P.shape[1], "fields_measured": nf_meas, "device_generation_s": t_gen,
            "download_s": t_down, "download_bytes": 8 * n * nf_meas, "numpy_plan_once_s": t_plan, "numpy_interpolation_s": t_interp,
            "upload_s": t_up, "upload_bytes": 8 * P.shape[1] * nf_meas, "ms_per_field": 1e3 * per_field,
            "extrapolated_to_fields": nf_total, "extrapolated_total_s": t_plan + per_field * nf_total,
            "note": "gsi_fftrf_fields, download, numpy restatement of FFTRF.interpolate on one core, upload; measured for "
                    "fields_measured fields and scaled to extrapolated_to_fields: an extrapolation"}


def time_getxis(ctx, Ns, P, nf, K, p, q):
    out = {"Ns": list(Ns), "points": P.shape[1], "fields": nf, "rank": K, "p": p, "q": q}
    for rep in range(2):
        t0 = time.perf_counter()
        op = gsi.lowrank_fftrf_operator(ctx, Ns, *ARGS, nf, seed=0, points=P)
        ctx.sync()
        out["operator_build_ms" if rep else "operator_build_ms_first"] = 1e3 * (time.perf_counter() - t0)
        op.close()
    t0 = time.perf_counter()
    basis = gsi.getxis_fftrf(Ns, *ARGS, nf, K, p, q, seed=0, ctx=ctx, device=True, points=P)
    ctx.sync()
    out["getxis_fftrf_total_ms_host_omega"] = 1e3 * (time.perf_counter() - t0)
    out["xi0_finite"] = bool(np.isfinite(basis[0]).all())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fftrf_unstructured.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    ctx = gsi.Context(0)
    if a.small:
        Ns, m, nf, reps, gx, nf_meas = (100, 100), 10_000, 16, 2, (8, 4, 2), 2
    else:
        Ns, m, nf, reps, gx, nf_meas = (1000, 1000), 1_000_000, 1024, 3, (256, 64, 2), 8
    P = np.asfortranarray(np.random.default_rng(0).random((len(Ns), m)))
    doc = {"what": __doc__.split("\n")[0] + " " + __doc__.split("\n")[1], "toy_sizes": bool(a.small)}
    doc["calls"] = time_calls(ctx, Ns, P, nf, reps)
    print(json.dumps(doc["calls"]), flush=True)
    ctx.release_cache()
    doc["replaced_path"] = time_replaced_path(ctx, Ns, P, nf, nf_meas)
    print(json.dumps(doc["replaced_path"]), flush=True)
    ctx.release_cache()
    doc["getxis"] = time_getxis(ctx, Ns, P, nf, *gx)
    print(json.dumps(doc["getxis"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
