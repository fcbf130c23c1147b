"""`gsi_op_solve_trace` / `gsi_slq_quadrature` / `gsi_precond_sample` / `gsi_precond_logdet` / `logdet` / `log_likelihood` on
the CPU reference library: the traced form of solvers.cpp's host driver (csrc/block_cg_host.hpp;
path 3, "composed") and csrc/slq_state.hpp's quadrature run on the host, against numpy.  Cases and checks:
tests/logdet_cases.py.  tests/test_op_logdet_gpu.py runs the same checks on csrc/block_slq.hip.
OP_LOGDET_ERRORS=<path>: the largest ratios seen, as profiles/op_logdet_errors.json."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import cpuref
import logdet_cases as lc
import pcg_cases as pg
import solve_cases as sc

PATH = "composed"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()
    path = os.environ.get("OP_LOGDET_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump({"library": "cpu reference, composed path, quadrature on the host",
                       "bars": {"quadrature": "max(4 x |float64 QL restatement - eigh|, 1e-13 x rho0 sum tau^2 |log lambda|)",
                                "sample, logdet_P": "4 x the float64 restatement's error, floor 1e-13",
                                "probes": "max(4 x the numpy restatement's error, 1e-12) x rho0",
                                "exact logdet": "1e-11 |slogdet|", "log_likelihood": "1e-10 relative"},
                       "largest_probe_ratio": max((v for k, v in lc.RATIOS.items() if k.startswith("probes")), default=0.0),
                       "ratios_to_the_bar": lc.RATIOS}, f, indent=1, sort_keys=True)
            f.write("\n")


def test_exported(gsi):
    for name in ("logdet", "log_likelihood", "solve_trace"):
        assert name in gsi.__all__ and callable(getattr(gsi, name)), name
    assert callable(gsi.Operator.logdet) and callable(gsi.Operator.log_likelihood)
    assert callable(gsi.Preconditioner.sample) and isinstance(gsi.Preconditioner.logdet, property)


def test_ql_restatement_against_eigh():
    """The float64 QL restatement the bars are built from agrees with eigh to 1e-12 of the scale on a 190-step trace."""
    al, be, r0 = lc.long_trace(190)
    v, scale = lc.gauss_eigh(al, be, 190, r0)
    assert abs(lc.ql_f64(al, be, 190, r0) - v) <= 1e-12 * scale


def test_quadrature_alone(cx):
    lc.quadrature_cases(cx)


@pytest.mark.parametrize("n,K,b", pg.APPLY)
def test_sample_and_logdet_P(gsi, cx, n, K, b):
    lc.sample_case(gsi, cx, n, K, b)


@pytest.mark.parametrize("n,b,diag,K", pg.DENSE)
def test_trace_is_passive(gsi, cx, n, b, diag, K):
    lc.passive_case(gsi, cx, n, b, diag, K, PATH)


@pytest.mark.parametrize("n,diag,K", lc.PROBE_CASES)
def test_probe_values(gsi, cx, n, diag, K):
    lc.probe_values(gsi, cx, n, diag, K, PATH)


@pytest.mark.parametrize("K", [0, 8])
def test_exact_logdet(gsi, cx, K):
    lc.exact_logdet(gsi, cx, K, PATH)


def test_truncation(gsi, cx):
    lc.truncation(gsi, cx, PATH)


@pytest.mark.parametrize("K", [0, 32])
def test_log_likelihood_dense(gsi, cx, K):
    n = 257
    P = sc.points(n, 2, seed=n)
    op, d, A = pg.dense_inputs(gsi, cx, n, 0.1)
    Z = pg.eig_basis(A, K) if K else None
    pc = gsi.lowrank_preconditioner(op, basis=Z, diag=d) if K else None
    try:
        lc.likelihood_case(gsi, cx, op, P, 0.1, pc, lc.precond_factor(Z, K, d, 0.0, n), f"log_likelihood dense n={n} K={K}")
    finally:
        if pc is not None:
            pc.close()
        op.close()


def test_log_likelihood_pointcov_pivoted_cholesky(gsi, cx):
    lc.likelihood_pivchol(gsi, cx)


def test_same_seed_same_normals(gsi, cx):
    lc.same_normals(gsi, cx)


def test_refusals(gsi, cx):
    lc.refusals(gsi, cx, PATH)


def test_host_checker(tmp_path):
    """csrc/slq_state.hpp as a program of its own under the address and undefined-behaviour sanitizers."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host check"
    exe = str(tmp_path / "slq_host_check")
    src = os.path.join(ROOT, "tests", "slq_host_check.cpp")
    inc = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "slq host ok" in r.stdout
