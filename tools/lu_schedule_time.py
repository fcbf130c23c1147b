#!/usr/bin/env python3
"""lu(Y).L of device-resident panels under block schedules (csrc/lu_schedule.hpp): uniform 64-column blocks, the chooser's
own list, and the minimum of the pass model for other per-block constants, forced through GSI_LU_SCHEDULE (read at every
factorization).  Phase timer, best of five; one JSON line per panel shape.
   python tools/lu_schedule_time.py [m,l ...]  [--constants 0,16,32,64]"""
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model_minimum(l, block_passes):
    """the pass model of DESIGN.md 4.2 with `block_passes` per block after the first; first list in dictionary order"""
    def block(jb, s):
        nl = (s + 7) // 8
        return 4 * nl * (nl - 1) + ((jb + 2 * s + block_passes) if jb > 0 else 0)

    @functools.lru_cache(maxsize=None)
    def best(jb):
        left = l - jb
        c = [(block(jb, s) + best(jb + s)[0], (s,) + best(jb + s)[1]) for s in (16, 32, 48, 64) if s < left]
        if left <= 64:
            c.append((block(jb, left), (left,)))
        return min(c)
    return list(best(0)[1])


def main():
    import gsi_amd as gsi
    shapes = [tuple(int(x) for x in a.split(",")) for a in sys.argv[1:] if not a.startswith("--")]
    shapes = shapes or [(1000000, 160), (1000000, 320), (65536, 160), (5000, 160)]
    consts = [0, 16, 32, 64]
    for a in sys.argv[1:]:
        if a.startswith("--constants"):
            consts = [int(x) for x in sys.argv[sys.argv.index(a) + 1].split(",")]
    ctx = gsi.Context(0)
    for m, l in shapes:
        legs = [("uniform64", {"GSI_LU_NB": "64"}), ("chosen", {})]
        legs += [("model_c%d" % c, {"GSI_LU_SCHEDULE": ",".join(str(s) for s in model_minimum(l, c))}) for c in consts]
        Y = gsi.DeviceMatrix(ctx, m, l)
        out = {"m": m, "l": l}
        for rnd in range(2):                      # the legs alternate: two rounds, the best of all repeats kept
            for tag, env in legs:
                for k in ("GSI_LU_SCHEDULE", "GSI_LU_NB"):
                    os.environ.pop(k, None)
                os.environ.update(env)
                ts = []
                for rep in range(5):
                    Y.randn(5)
                    ctx.sync(); ctx.profile(True); ctx.phase_reset()
                    gsi.lu_L_dev(Y)
                    ph = ctx.phase_times(); ctx.profile(False)
                    ts.append(ph["lu"][0])
                rec = out.setdefault(tag, {"schedule": env.get("GSI_LU_SCHEDULE", env.get("GSI_LU_NB", "default")), "ms": min(ts)})
                rec["ms"] = round(min(rec["ms"], min(ts)), 4)
        print(json.dumps(out), flush=True)
        Y.close(); ctx.release_cache()


if __name__ == "__main__":
    main()
