"""bench.py --dump-outputs: what the timed path returned in its last step, as DIR/<name>.npy, the same from run to run, so
that two builds can be compared output for output.  The helpers are checked on the CPU; one small end-to-end run of bench.py
(twice, same arguments) on the GPU."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_row_sample_is_fixed_and_within_budget():
    b = _bench()
    n, l = 1000000, 320
    r1, r2 = b.dump_row_sample(n, l), b.dump_row_sample(n, l)
    assert np.array_equal(r1, r2)
    assert np.all(np.diff(r1) > 0) and r1[0] >= 0 and r1[-1] < n
    assert 8 * l * (r1.size + 1) <= b.DUMP_BYTES < 64 * 10**6
    assert np.array_equal(b.dump_row_sample(1000, 24), np.arange(1000))      # small outputs are written whole


class _FakeRanks:
    """One rank of a G-rank job whose host all-gather returns the parts recorded for all ranks."""

    def __init__(self, rank, world, parts):
        self.r, self.g, self.parts = rank, world, parts

    def rank(self):
        return self.r, self.g

    def shard(self, m):
        pad = -(-m // self.g)
        row0 = min(self.r * pad, m)
        return row0, min(pad, m - row0)

    def host_allgather(self, values):
        self.parts[self.r] = np.array(values, dtype=np.float64)
        if len(self.parts) < self.g:
            return np.zeros((self.g, len(values)))
        return np.stack([self.parts[k] for k in range(self.g)])


@pytest.mark.parametrize("world", [1, 3])
def test_gather_rows_of_a_row_sharded_z(world):
    b = _bench()
    n, l = 1001, 7
    Z = np.random.default_rng(1).standard_normal((n, l))
    rows = np.array([0, 5, 333, 334, 335, 667, 668, 1000])
    parts = {}
    got = None
    for r in list(range(1, world)) + [0]:              # rank 0 last: by then every other rank's part is recorded
        ctx = _FakeRanks(r, world, parts)
        row0, nloc = ctx.shard(n)
        got = b.gather_rows(ctx, Z[row0:row0 + nloc], n, rows)
    assert np.array_equal(got, Z[rows])


def test_write_outputs(tmp_path):
    b = _bench()
    b.write_outputs(str(tmp_path / "out"), {"S": [3.0, 2.0], "Z_rows": np.asfortranarray(np.ones((4, 2), np.float32))})
    S, Z = np.load(tmp_path / "out" / "S.npy"), np.load(tmp_path / "out" / "Z_rows.npy")
    assert S.dtype == np.float64 and Z.dtype == np.float64 and Z.shape == (4, 2) and list(S) == [3.0, 2.0]


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_exactly(tmp_path):
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--n", "20000", "--samples", "64", "--K", "16", "--p", "8",
            "--q", "1", "--no-secondary", "--no-boundary", "--no-cpu-baseline"]
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GSI_BENCH_RDV"):
        env.pop(k, None)
    outs = []
    for run in ("a", "b"):
        d = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        outs.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = outs
    assert sorted(a) == ["S", "Z_rows"]
    assert a["S"].shape == (24,) and a["Z_rows"].shape == (20000, 24)
    assert np.all(np.isfinite(a["Z_rows"])) and np.all(a["S"][:16] > 0)
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
