"""The bilinear reduction of the likelihood gradient on the CPU reference library: `gsi_mat_bilinear`
through csrc/bilinear_terms_host.hpp (that backend declines `Backend::bilinear_terms`), bit for bit against
tests/bilinear_model.py; the refusals; and the host header alone under the sanitizers.  Cases: tests/bilinear_cases.py."""
import os
import shutil
import subprocess

import pytest

import bilinear_cases as bc
import cpuref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _feature_present(gsi):
    """These files restate product code (csrc/pointcov.hpp's `dprofile`, csrc/bilinear_terms_host.hpp's order, the formulas of
    `log_likelihood_grad`): beside a library without it they check nothing, so they fail there."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "geostatinversion.jl_amd", "csrc")
    assert "dprofile" in open(os.path.join(csrc, "pointcov.hpp")).read()
    assert os.path.exists(os.path.join(csrc, "bilinear_terms_host.hpp"))
    for name in ("log_likelihood_grad", "fit_covariance", "mat_bilinear", "fft_gridcov_derivative"):
        assert name in gsi.__all__, name


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()


def test_exported(gsi):
    for name in ("mat_bilinear", "op_bilinear_terms"):
        assert name in gsi.__all__ and callable(getattr(gsi, name)), name
    for name in ("gsi_mat_bilinear", "gsi_op_bilinear_terms", "gsi_mat_copy_cols"):
        assert name in gsi._lib.SIGNATURES, name


def test_model_is_ordered():
    bc.run_model_is_ordered()


@pytest.mark.parametrize("n", bc.ROWS)
def test_bits(gsi, cx, n):
    for b, g in bc.SHAPES:
        bc.run_case(gsi, cx, n, b, g)


def test_refusals(gsi, cx):
    bc.run_refusals(gsi, cx)


def test_host_code_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host-path check"
    exe = str(tmp_path / "bilinear_host_check")
    src = os.path.join(ROOT, "tests", "bilinear_host_check.cpp")
    inc = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bilinear host ok" in r.stdout
