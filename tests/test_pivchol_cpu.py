"""`gsi_op_pivoted_cholesky` / `RandMatFact.pivoted_cholesky` / `principal_factor` / `getxis_pivchol` /
`lowrank_preconditioner(method="pivoted_cholesky")` on the CPU reference library: the host path of
csrc/pivoted_chol_host.hpp around csrc/pchol_state.hpp (path 3, "composed": columns by the operator product with a unit
vector), against the numpy model tests/pivchol_model.py.  Cases and checks: tests/pivchol_cases.py;
tests/test_pivchol_gpu.py runs the same checks on csrc/pivoted_chol.hip.

Not run here: the 257 x 256 grid.  Its edge -- more partials than the deciding workgroup takes in one sweep -- exists in
the kernels only, and a column of that operator by a product with a unit vector is 4.3e9 table lookups on the CPU.  The
preconditioned solve runs on 300 points here and on the issue's 2000 on the device.
PIVCHOL_ERRORS=<path>: the attained figures, as profiles/pivchol_errors.json."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import cpuref
import pivchol_cases as pv
import pivchol_model as pm
import solve_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = "composed"
_KEEP = []


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()
    path = os.environ.get("PIVCHOL_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump({"library": "cpu reference, composed path", "cases": pv.ERRORS}, f, indent=1, sort_keys=True)
            f.write("\n")


def test_exported(gsi):
    for name in ("pivoted_cholesky", "principal_factor", "getxis_pivchol"):
        assert name in gsi.__all__ and callable(getattr(gsi, name)), name
    assert gsi.RandMatFact.pivoted_cholesky is gsi.pivoted_cholesky
    assert gsi.RandMatFact.principal_factor is gsi.principal_factor
    import inspect
    sig = inspect.signature(gsi.lowrank_preconditioner).parameters
    assert sig["method"].default == "randsvd" and sig["tol"].default == 0.0
    assert sig["method"].kind is inspect.Parameter.KEYWORD_ONLY and sig["tol"].kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("gsi_op_pivoted_cholesky", "gsi_mat_principal_factor"):
        assert name in gsi._lib.SIGNATURES


def test_model_on_a_matrix_worked_by_hand():
    """[[4, 2], [2, 2]]: pivot 0, L[:, 0] = (2, 1), d = (0, 1); pivot 1, L[1, 1] = 1."""
    r = pm.pivchol(*pm.matrix_source(np.array([[4.0, 2.0], [2.0, 2.0]])), 2)
    assert r["piv"].tolist() == [0, 1] and np.array_equal(r["L"], [[2.0, 0.0], [1.0, 1.0]])
    assert (r["rank"], r["reason"], r["trace0"], r["trace"], r["dmax"]) == (2, 3, 6.0, 0.0, 0.0)
    assert r["gaps"].tolist() == [0.5, 1.0]
    # a tie: the lowest index
    r = pm.pivchol(*pm.matrix_source(np.array([[1.0, 0.5, 0.0], [0.5, 2.0, 0.5], [0.0, 0.5, 2.0]])), 1)
    assert r["piv"].tolist() == [1] and r["reason"] == 1 and r["gaps"].tolist() == [0.0]


@pytest.mark.parametrize("n,K", pv.DENSE)
def test_parity_dense(gsi, cx, n, K):
    pv.parity_dense(gsi, cx, n, K, PATH)


@pytest.mark.parametrize("nx,ny,K", pv.TABLE)
def test_parity_table(gsi, cx, nx, ny, K):
    pv.parity_table(gsi, cx, nx, ny, K, PATH)


def test_parity_gridcov_kinds(gsi, cx):
    """The other two creators of the implicit grid covariance make the same kind of operator: their table is read back by a
    product with the identity."""
    for kind in (0, 1):
        op = gsi.gridcov_implicit_operator(cx, 9, 7, 2.5, kind=kind)
        try:
            A = np.asfortranarray(op.matmul(np.eye(63)))
            ref = pm.pivchol(*pm.matrix_source(A), 20)
            pv.check_against_model(f"gridcov kind {kind}", pv.factor(gsi, op, 20), ref, PATH)
        finally:
            op.close()


def test_host_matrix_in_host_factor_out(gsi, cx):
    pv.host_matrix_in_host_factor_out(gsi, cx, PATH)


def test_stopping(gsi, cx):
    pv.stopping(gsi, cx, PATH)


def test_refusals(gsi, cx):
    other = gsi.Context(0, lib=cx.lib)
    try:
        pv.refusals(gsi, cx, other)
    finally:
        other.close()


def test_refuses_a_communicator(gsi, monkeypatch):
    lib = cpuref.load_cpuref()
    cbs = (cpuref.ALLREDUCE_FN(lambda buf, count: None),
           cpuref.ALLGATHER_FN(lambda send, recv, count: [recv.__setitem__(i, send[i]) for i in range(count)] and None))
    _KEEP.extend(cbs)                      # the library keeps the pointers
    lib.gsi_cpuref_set_collectives(*cbs)
    monkeypatch.setenv("GSI_FORCE_COMM", "1")
    cc = gsi.Context(0, lib=lib)
    try:
        cc.comm_init(1, 0, b"\0" * 128)
        op = gsi.dense_operator(cc, np.eye(4))
        sc.refused(gsi, lambda: gsi.pivoted_cholesky(op, 2), "communicator")
        Lm = gsi.DeviceMatrix(cc, 4, 2)
        sc.refused(gsi, lambda: gsi.principal_factor(Lm), "communicator")
        Lm.close()
        op.close()
    finally:
        cc.close()


@pytest.mark.parametrize("kind,d,nugget,seed", pv.SCATTERED)
def test_scattered_points(gsi, cx, kind, d, nugget, seed):
    pv.scattered(gsi, cx, kind, d, nugget, seed, PATH)


def test_identities(gsi, cx):
    pv.identities_dense_table(gsi, cx, PATH)


def test_preconditioner(gsi, cx):
    pv.preconditioner(gsi, cx, PATH, n=300)


def test_principal_factor(gsi, cx):
    pv.principal(gsi, cx)


@pytest.mark.parametrize("M,N,mu", [(2, 16, 10.0), (8, 64, 0.0), (16, 256, 10.0)])
@pytest.mark.parametrize("principal", [True, False])
def test_getxis_pivchol_feeds_pcgadirect(gsi, cx, M, N, mu, principal):
    pv.pcga_end_to_end(gsi, cx, M, N, mu, principal)


# ---- the host path as a program of its own, under sanitizers ----------------------------------------------------------
def test_host_path_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host-path check"
    exe = str(tmp_path / "pivchol_host_check")
    src = os.path.join(ROOT, "tests", "pivchol_host_check.cpp")
    inc = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pivchol host ok" in r.stdout
