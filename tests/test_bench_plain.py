"""A plain `bench.py --gpus N --steps K --warmup W` does what its headline figure needs and nothing else; what takes runs of
its own (secondary workloads, host boundary, CPU oracle and parity, and for N > 1 the skew-split step, the one-GPU re-run and
the row-sharded implicit step) comes with --full, where the --no-* options leave parts out.  The option logic on the CPU;
one small one-rank run and one two-rank rehearsal on the GPU."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("no_cpu_baseline", "no_secondary", "no_boundary", "no_full_parity", "no_implicit")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_leaves_out_every_extra():
    a = _bench().parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.steps == 20 and a.warmup == 5
    assert all(getattr(a, k) for k in EXTRAS), vars(a)


def test_full_runs_every_extra_unless_left_out():
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert a.full is True and not any(getattr(a, k) for k in EXTRAS) and not a.no_fft_512cube, vars(a)
    a = b.parse_args(["--full", "--no-boundary", "--no-cpu-baseline"])
    assert a.no_boundary and a.no_cpu_baseline and not a.no_secondary and not a.no_full_parity and not a.no_implicit


def _run(args, extra_env=None, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GSI_BENCH_RDV"):
        env.pop(k, None)
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


def _assert_plain_line(out, steps, warmup):
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["unit"] == "GB/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["full"] is False and out["cpu_baseline"] is None
    for k in ("secondary", "boundary", "parity_full_size", "parity_cpu_sample", "sv_rel_err", "multi_rank_vs_one_gpu"):
        assert k not in out, k
    assert out["phases_ms_skew_split_one_step"] is None
    assert out["phases_ms_per_step"]["gemm_n"] > 0 and out["roofline"]["launches"] > 0


@pytest.mark.gpu
def test_plain_run_line(tmp_path):
    out = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--n", "20000", "--samples", "64", "--K", "16", "--p", "8",
                "--q", "1"], timeout=300)
    _assert_plain_line(out, 3, 1)
    assert out["n_gpus"] == 1 and out["config"]["n"] == 20000


@pytest.mark.gpu
@pytest.mark.skipif(bool(os.environ.get("GSI_SKIP_BENCH_MULTIRANK")), reason="GSI_SKIP_BENCH_MULTIRANK set")
def test_plain_two_rank_rehearsal_line():
    # the headline size of tests/test_bench_multirank_gpu.py, both ranks on GPU 0: timed steps and per-rank phases only
    out = _run(["--gpus", "2", "--steps", "2", "--warmup", "1"], {"GSI_BENCH_ONE_GPU": "1"})
    _assert_plain_line(out, 2, 1)
    assert out["n_gpus"] == 2 and out["config"]["n"] == 1000000
    assert out["path_counters"]["n_ranks_seen"] == 2 and out["path_counters"]["lu_form_same_on_all_ranks"] is True
    assert out["phases_ms_max_min_over_ranks"]["gemm_n"]["max"] > 0
