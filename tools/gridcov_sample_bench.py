#!/usr/bin/env python3
"""What sampling Gaussian fields with a grid covariance function costs on the device (csrc/gridcov_sample.hip), against the
FFTRF power-law sampler on the same grid in the same process.

Writes one JSON document (default profiles/gridcov_sample.json).  Every number says what it is:
  * `call_ms_per_field`: a host clock around `gsi_gridcov_fields` in seed mode, ended by a device synchronise -- the randn fill
    of the noise and the passes, NOT a kernel time from a trace;
  * `bytes_per_field`: computed from the shapes (below) for the passes alone; `bytes_per_field_with_fill` adds the randn
    fill's writes, and `gb_per_s` = those bytes over that time;
  * `fftrf`: `tools/fftrf_sample_bench.py`'s measurement of `gsi_fftrf_fields` on the same grid, taken here, in this
    process; `ratio_to_fftrf` = this sampler's per-field time over FFTRF's (below 1: faster);
  * `plan_ms`: a host clock around `gsi_gridcov_sampler_create` (lag table, transform, statistics and their read-back), the
    second creation of that plan.
  python3 tools/gridcov_sample_bench.py [--out PATH] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gsi_amd as gsi  # noqa: E402
import fftrf_sample_bench as fb  # noqa: E402


def bytes_per_pair(N, M):
    """HBM bytes one pair of fields must move in the passes: amp and the two noise arrays read by the first pass, every pass's
    complex reads and writes with the crop behind each axis, two destination columns written once."""
    mtot, n = int(np.prod(M)), int(np.prod(N))
    b = 24 * mtot
    cur = list(M)
    for a in range(len(N)):
        if a > 0:
            b += 16 * int(np.prod(cur))                # read the cropped array of the previous pass
        cur[a] = N[a]
        if a < len(N) - 1:
            b += 16 * int(np.prod(cur))
    return b + 16 * n


def time_fields(ctx, Ns, nf, reps, embed=None, **cov):
    t0 = time.perf_counter()
    s = gsi.gridcov_sampler(ctx, Ns, embed=embed, **cov)
    plan_first = time.perf_counter() - t0
    s.close()
    t0 = time.perf_counter()
    s = gsi.gridcov_sampler(ctx, Ns, embed=embed, **cov)
    plan_ms = 1e3 * (time.perf_counter() - t0)
    F = gsi.DeviceMatrix(ctx, int(np.prod(Ns)), nf)

    def run(seed):
        gsi._lib.check(ctx.lib.gsi_gridcov_fields(ctx.h, s.h, F.h, None, 0, seed, 0), ctx.lib)
        ctx.sync()

    run(1)                                             # warm-up: code objects, workspace
    ts = []
    for r in range(reps):
        t0 = time.perf_counter()
        run(2 + r)
        ts.append(time.perf_counter() - t0)
    col = F.to_host()[:, :1] if nf <= 4 else None
    F.close()
    bpf = bytes_per_pair(Ns, s.M) / 2
    fill = 16 * s.Mtot / 2
    ms = [1e3 * t / nf for t in ts]
    out = {"Ns": list(Ns), "M": list(s.M), "cov": {k: (list(v) if np.ndim(v) else v) for k, v in cov.items()}, "fields": nf,
           "repeats": reps, "neg_mass": s.neg_mass, "lam_min_over_lam_max": s.lam_min / s.lam_max, "clamped": s.clamped,
           "plan_ms": plan_ms, "plan_ms_first": 1e3 * plan_first, "call_ms_per_field": {"median": float(np.median(ms)), "all": ms},
           "bytes_per_field": bpf, "bytes_per_field_with_fill": bpf + fill,
           "gb_per_s": (bpf + fill) / (float(np.median(ms)) * 1e-3) / 1e9, "launches_per_batch": len(Ns)}
    s.close()
    return out, col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gridcov_sample.json"))
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--only", type=int, default=None, help="run one workload only (0, 1, 2) and no FFTRF yardstick: for a trace")
    a = ap.parse_args()
    ctx = gsi.Context(0)
    if a.small:
        work = [((100, 100), 16, None, dict(kind="exponential", ell=10.0)),
                ((100, 100), 16, (512, 512), dict(kind="exponential", ell=10.0)),
                ((16, 16, 16), 8, None, dict(kind="exponential", ell=2.0))]
    else:
        work = [((1000, 1000), 1024, None, dict(kind="exponential", ell=100.0)),
                ((1000, 1000), 1024, (4096, 4096), dict(kind="exponential", ell=100.0)),
                ((128, 128, 128), 256, None, dict(kind="exponential", ell=8.0))]
    doc = {"what": __doc__.split("\n")[0], "toy_sizes": bool(a.small), "workloads": []}
    yard = {}
    for i, (Ns, nf, embed, cov) in enumerate(work):
        if a.only is not None and i != a.only:
            continue
        r, _ = time_fields(ctx, Ns, nf, 3, embed=embed, **cov)
        ctx.release_cache()
        if a.only is None:
            if Ns not in yard:                          # the yardstick: FFTRF's sampler, same grid, same process
                yard[Ns], _ = fb.time_fields(ctx, Ns, nf, 3)
                ctx.release_cache()
            y = yard[Ns]
            r["fftrf"] = {k: y[k] for k in ("call_ms_per_field", "bytes_per_field", "gb_per_s")}
            r["ratio_to_fftrf"] = r["call_ms_per_field"]["median"] / y["call_ms_per_field"]["median"]
        print(json.dumps({k: r[k] for k in ("Ns", "M", "fields", "plan_ms", "call_ms_per_field", "gb_per_s", "neg_mass")
                          + (("ratio_to_fftrf",) if "ratio_to_fftrf" in r else ())}), flush=True)
        doc["workloads"].append(r)
    if a.only is None:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
