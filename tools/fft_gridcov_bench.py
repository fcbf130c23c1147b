#!/usr/bin/env python3
"""The FFT operator for covariance functions (gsi_op_fft_gridcov) at the headline size, on the GPU box:
    timeout -k 10 900 python tools/fft_gridcov_bench.py [--out profiles/fft_gridcov_1e6.json]
ONE process, 1000 x 1000 grid, exponential kernel, ell = 100:
  (a) the 320-column product of the new operator and of fft_powerlaw_operator on the same grid, two plans of each,
      alternated: the passes are the same kernels, so the new operator's median must lie within the spread of the
      power-law operator's own samples -- that operator is the yardstick, not the code under test (a gap beyond it means
      the plan or its layout differs: a defect);
  (b) randsvd K = 256, p = 64, q = 2 through the new operator, with the phase times;
  (c) one 16-column product of gridcov_implicit_operator(kind=1) on the same X: its time, max|Y_fft - Y_implicit| / max|Y|,
      then one 320-column product of it, from which the implicit operator's randsvd time is DERIVED (six such products;
      marked as derived).
Every step runs under a time limit of its own (a watchdog that ends the process: nothing is started on the GPU after a
step that hung), and an exception in one step ends the run."""
import argparse, json, os, sys, threading, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gsi_amd as gsi

ap = argparse.ArgumentParser()
ap.add_argument("--g", type=int, default=1000)
ap.add_argument("--ell", type=float, default=100.0)
ap.add_argument("--l", type=int, default=320)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=5, help="products per timing")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fft_gridcov_1e6.json"))
a = ap.parse_args()


class step:
    """`with step(name, seconds):` -- the process ends (status 124) if the block is still running after `seconds`."""
    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds
    def __enter__(self):
        print(f"[{self.name}] (limit {self.seconds} s)", flush=True)
        self.t = threading.Timer(self.seconds, lambda: (print(f"[{self.name}] time limit: ending the run", flush=True), os._exit(124)))
        self.t.daemon = True
        self.t.start()
    def __exit__(self, *exc):
        self.t.cancel()
        return False


g, l = a.g, a.l
n = g * g
ctx = gsi.Context(0)
lib = ctx.lib
res = {"grid": [g, g], "n": n, "kernel": "exponential", "ell": a.ell, "l": l, "hipcc": None}


def mul(op, X, Y):
    gsi._lib.check(lib.gsi_op_mul_dev(ctx.h, op.h, 0, X.h, Y.h), lib)


def timed(op, X, Y, reps):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        mul(op, X, Y)
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


with step("plans", 120):
    t0 = time.perf_counter()
    op = gsi.fft_gridcov_operator(ctx, [g, g], kind="exponential", ell=a.ell)
    ctx.sync()
    res["plan_ms_first"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    gsi.fft_gridcov_operator(ctx, [g, g], kind="exponential", ell=a.ell).close()
    ctx.sync()
    res["plan_ms"] = (time.perf_counter() - t0) * 1e3
    # TWO plans of each operator, created in the order new, power-law, power-law, new: where a plan's spectrum and work
    # array lie in HBM is part of what a product time depends on, so the yardstick -- the power-law operator's own
    # spread -- has to contain it, and the new operator must not be compared through one placement only
    pl = gsi.fft_powerlaw_operator(ctx, [g, g], -3.5)
    pl2 = gsi.fft_powerlaw_operator(ctx, [g, g], -3.5)
    op2 = gsi.fft_gridcov_operator(ctx, [g, g], kind="exponential", ell=a.ell)
    X = gsi.DeviceMatrix(ctx, n, l).randn(1)
    Y = gsi.DeviceMatrix(ctx, n, l)
    ops = [("fft_gridcov#1", op), ("fft_powerlaw#1", pl), ("fft_powerlaw#2", pl2), ("fft_gridcov#2", op2)]
    for _, o in ops:
        timed(o, X, Y, a.reps)                         # one untimed round: code objects, clocks

with step("a: alternated products", 180):
    t = {name: [] for name, _ in ops}
    for r in range(a.rounds):
        for i in range(len(ops)):                      # the order rotates from round to round
            name, o = ops[(i + r) % len(ops)]
            t[name].append(timed(o, X, Y, a.reps))
    t_new = t["fft_gridcov#1"] + t["fft_gridcov#2"]
    t_pl = t["fft_powerlaw#1"] + t["fft_powerlaw#2"]
    med_new, med_pl = float(np.median(t_new)), float(np.median(t_pl))
    # the yardstick is the power-law operator alone (both of its plans): its spread, not the new operator's own
    spread_pl = max(t_pl) - min(t_pl)
    gap = abs(med_new - med_pl)
    res["product"] = {"columns": l, "rounds": a.rounds, "products_per_timing": a.reps, "ms": t,
                      "median_ms": {k: float(np.median(v)) for k, v in t.items()},
                      "fft_gridcov_median_ms": med_new, "fft_powerlaw_median_ms": med_pl,
                      "fft_powerlaw_range_ms": [min(t_pl), max(t_pl)], "fft_gridcov_range_ms": [min(t_new), max(t_new)],
                      "fft_powerlaw_spread_ms": spread_pl,
                      "fft_powerlaw_plan_to_plan_ms": abs(float(np.median(t["fft_powerlaw#1"])) - float(np.median(t["fft_powerlaw#2"]))),
                      "fft_gridcov_plan_to_plan_ms": abs(float(np.median(t["fft_gridcov#1"])) - float(np.median(t["fft_gridcov#2"]))),
                      "gap_ms": gap, "gap_relative": gap / med_pl, "within_fft_powerlaw_spread": bool(gap <= spread_pl)}
    for k, v in t.items():
        print(f"  {k}: median {np.median(v):.3f} ms [{min(v):.3f}, {max(v):.3f}]", flush=True)
    print(f"  {l} columns: fft_gridcov median {med_new:.3f} ms, fft_powerlaw median {med_pl:.3f} ms: gap {gap:.3f} ms "
          f"({100 * gap / med_pl:.2f} %), fft_powerlaw spread {spread_pl:.3f} ms -> "
          f"{'within' if gap <= spread_pl else 'BEYOND'} the yardstick's spread", flush=True)
    pl.close(); pl2.close(); op2.close()

with step("b: randsvd", 240):
    K, p, q = 256, 64, 2
    assert K + p == l
    Z = gsi.DeviceMatrix(ctx, n, l)
    S = gsi.DeviceMatrix(ctx, l, 1)
    gsi._lib.check(lib.gsi_randsvd_dev(ctx.h, op.h, X.h, K, p, q, Z.h, S.h), lib)      # warm-up
    ctx.sync()
    runs, phases = [], None
    for _ in range(5):
        ctx.profile(True); ctx.phase_reset()
        t0 = time.perf_counter()
        gsi._lib.check(lib.gsi_randsvd_dev(ctx.h, op.h, X.h, K, p, q, Z.h, S.h), lib)
        ctx.sync()
        runs.append((time.perf_counter() - t0) * 1e3)
        phases = {k: round(v[0], 2) for k, v in ctx.phase_times().items() if v[0] > 0}
        ctx.profile(False)
    Sh = S.to_host()[:, 0]
    res["randsvd"] = {"K": K, "p": p, "q": q, "ms": runs, "median_ms": float(np.median(runs)), "phases_ms_last_run": phases,
                      "S0": float(Sh[0]), "SK_over_S0": float(Sh[K - 1] / Sh[0])}
    print(f"  randsvd K={K} p={p} q={q}: {runs} ms, phases {phases}", flush=True)
    Z.close(); S.close()

with step("c: the implicit operator on the same X", 180):
    lc = 16
    Xc = gsi.DeviceMatrix(ctx, n, lc).randn(2)
    Yf = gsi.DeviceMatrix(ctx, n, lc)
    Yi = gsi.DeviceMatrix(ctx, n, lc)
    mul(op, Xc, Yf)
    impl = gsi.gridcov_implicit_operator(ctx, g, g, a.ell, kind=1)
    mul(impl, Xc, Yi)                                  # warm-up (code objects)
    t_impl = timed(impl, Xc, Yi, 1)
    A, B = Yf.to_host(), Yi.to_host()
    err = float(np.abs(A - B).max() / np.abs(B).max())
    # one product of the full 320-column sketch (about 10 s): the implicit kernel generates every entry once per 160-column
    # tile, so the 16-column time does not scale by 320 / 16; randsvd applies the operator 2 q + 2 times
    t_impl_l = timed(impl, X, Y, 1)
    nprod = 2 * q + 2
    res["implicit"] = {"columns": lc, "product_ms": t_impl, "max_abs_diff_over_max_abs_Y": err,
                       "product_ms_full_sketch": t_impl_l, "randsvd_products": nprod,
                       "randsvd_ms_derived_from_products_only": t_impl_l * nprod,
                       "note": "derived: one timed 320-column product x six products; panel phases not included"}
    res["randsvd"]["ratio_implicit_derived_over_fft"] = res["implicit"]["randsvd_ms_derived_from_products_only"] / res["randsvd"]["median_ms"]
    print(f"  implicit {lc} columns: {t_impl:.1f} ms; max|Y_fft - Y_implicit| / max|Y| = {err:.2e}; {l} columns: {t_impl_l:.0f} ms; "
          f"derived implicit randsvd {res['implicit']['randsvd_ms_derived_from_products_only'] / 1e3:.1f} s = "
          f"{res['randsvd']['ratio_implicit_derived_over_fft']:.0f} x", flush=True)
    Y.close(); X.close()
    impl.close(); op.close()

vfile = os.path.join(os.path.dirname(os.path.abspath(gsi.__file__)), "build", "hipcc_version.txt")
res["hipcc"] = open(vfile).read().strip() if os.path.exists(vfile) else None
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("wrote", a.out)
