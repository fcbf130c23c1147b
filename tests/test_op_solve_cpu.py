"""`gsi_op_solve_cg` / `Operator.solve` / `kriging_weights` on the CPU reference library: the host driver of solvers.cpp
with cg_state.hpp's recurrences composed from the backend's BLAS-1 primitives (path 3, "composed"), against numpy.  Cases,
bars and checks: tests/solve_cases.py.  tests/test_op_solve_gpu.py runs the same checks on the fused device kernels."""
import numpy as np
import pytest

import cpuref
import solve_cases as sc

PATH = "composed"
_KEEP = []


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()


def test_exported(gsi):
    for name in ("solve", "kriging_weights", "krige_to_grid", "condition_fields", "mat_axpy"):
        assert name in gsi.__all__ and callable(getattr(gsi, name)), name
    assert callable(gsi.Operator.solve)


def _all_cases(gsi, cx):
    for n, b, diag in sc.DENSE:
        yield f"dense n={n} b={b} diag={diag}", (lambda n=n, diag=diag: sc.dense_case(gsi, cx, n, diag)), b
    yield "pointcov 2-D n=300", (lambda: sc.pointcov_case(gsi, cx, 2)), 2
    yield "pointcov 3-D n=300", (lambda: sc.pointcov_case(gsi, cx, 3)), 3
    yield "lowrank N=40 n=200", (lambda: sc.lowrank_case(gsi, cx)), 16
    yield "fft powerlaw 12x9", (lambda: sc.powerlaw_case(gsi, cx)), 17


def test_inputs_are_fair(gsi, cx):
    """The condition behind the factor 2 of the residual bar: on every case a plain numpy CG ends within 1 tol (true
    residual), so what a solver adds beyond that is its own."""
    for name, make, b in _all_cases(gsi, cx):
        op, d = make()
        try:
            n = op.shape[0]
            M = sc.dense_of(op, d)
            B = sc.rhs(n, min(b, 3), seed=n + b)
            X, its = sc.numpy_cg(0.5 * (M + M.T), B, sc.TOL, 10 * n)
            rho = sc.true_relres(M, X, B)
            print(f"{name}: numpy CG {its.max()} iterations, true relres {rho.max():.3e}")
            assert (rho <= sc.TOL).all(), (name, rho.max())
        finally:
            op.close()


@pytest.mark.parametrize("n,b,diag", sc.DENSE)
def test_dense(gsi, cx, n, b, diag):
    op, d = sc.dense_case(gsi, cx, n, diag)
    try:
        sc.run_case(gsi, op, d, b, f"dense n={n} b={b} diag={diag}", PATH)
    finally:
        op.close()


@pytest.mark.parametrize("which", ["pointcov2", "pointcov3", "lowrank", "powerlaw"])
def test_operators(gsi, cx, which):
    make, b = {"pointcov2": (lambda: sc.pointcov_case(gsi, cx, 2), 2), "pointcov3": (lambda: sc.pointcov_case(gsi, cx, 3), 3),
               "lowrank": (lambda: sc.lowrank_case(gsi, cx), 16), "powerlaw": (lambda: sc.powerlaw_case(gsi, cx), 17)}[which]
    op, d = make()
    try:
        sc.run_case(gsi, op, d, b, which, PATH)
    finally:
        op.close()


def test_device_matrix_in_device_matrix_out(gsi, cx):
    op, d = sc.dense_case(gsi, cx, 65, "vec")
    B = sc.rhs(65, 3)
    Bd = gsi.DeviceMatrix.from_host(cx, B)
    try:
        Xd, rep = op.solve(Bd, diag=d, return_info=True)
        assert isinstance(Xd, gsi.DeviceMatrix) and rep["path"] == PATH
        Xh = op.solve(B, diag=d)
        assert np.array_equal(Xd.to_host(), Xh)
        assert np.array_equal(Bd.to_host(), B)                # B is not modified
        x1 = op.solve(B[:, 0], diag=d)
        assert x1.shape == (65,) and np.array_equal(x1, Xh[:, 0])
        Xd.close()
    finally:
        Bd.close()
        op.close()


def test_special_columns(gsi, cx):
    sc.special_columns(gsi, cx, PATH)


def test_determinism(gsi, cx):
    sc.determinism(gsi, cx, PATH)


def test_budget(gsi, cx):
    sc.budget(gsi, cx, PATH)


def test_breakdown(gsi, cx):
    sc.breakdown(gsi, cx, PATH)


def test_refusals(gsi, cx):
    sc.refusals(gsi, cx, PATH)


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
        sc.refused(gsi, lambda: op.solve(np.ones(4)), "communicator")
        op.close()
    finally:
        cc.close()


def test_mat_axpy(gsi, cx):
    sc.mat_axpy_cases(gsi, cx)


def test_kriging_weights_with_drift(gsi, cx):
    P = sc.points(150, 2, seed=21)
    op = gsi.pointcov_implicit_operator(cx, P, kind="exponential", ell=0.3)
    try:
        sc.kriging_drift(gsi, cx, op, P, 0.1, "kriging drift, pointcov m=150")
    finally:
        op.close()
