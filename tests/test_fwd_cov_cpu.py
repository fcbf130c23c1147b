"""The adjoint of a linear forward model, the operator H C H' and the linear inversion on the CPU reference library: the host
paths of pcga.cpp (fwd_adjoint_host.hpp, the CSR loop) under pipeline.cpp's fwd_cov_mul, with `fft_powerlaw_operator` as C
(that backend has no grid-covariance plan).  Cases, bars and checks: tests/fwd_cov_cases.py, tests/fwd_adjoint_model.py.
tests/test_fwd_adjoint_gpu.py and tests/test_fwd_cov_gpu.py run the kernels."""
import numpy as np
import pytest

import cpuref
import fwd_adjoint_model as fm
import fwd_cases
import fwd_cov_cases as fc
import solve_cases as sc

PATH = "composed"
_KEEP = []


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()


@pytest.fixture(scope="module", params=list(fc.POWERLAW))
def case(gsi, cx, request):
    """(name, Ns, grid operator, its dense matrix, dense H)"""
    Ns, beta = fc.POWERLAW[request.param]
    gop = gsi.fft_powerlaw_operator(cx, list(Ns), beta)
    n = int(np.prod(Ns))
    Cm = gop.matmul(np.eye(n))                     # existing code, not under test here
    yield request.param, Ns, gop, 0.5 * (Cm + Cm.T), fc.dense_H(Ns)
    gop.close()


def test_exported(gsi):
    for name in ("LinearDataOperator", "linear_data_operator", "estimate_field", "linear_inversion", "condition_on_linear_data"):
        assert name in gsi.__all__ and callable(getattr(gsi, name)), name
    for name in ("apply_dev", "adjoint", "adjoint_info"):
        assert callable(getattr(gsi.LinearForwardModel, name)), name


def test_inputs_are_fair(case):
    """Every solve case of this file: numpy's own CG ends with a true relative residual <= 1 tol."""
    name, Ns, _, Cm, H = case
    fc.fair(name, H @ Cm @ H.T + fc.NOISE * np.eye(H.shape[0]))


@pytest.mark.parametrize("gname", list(fc.GRIDCOV))
def test_inputs_of_the_gpu_file_are_fair(gname):
    """The same for the solve cases of tests/test_fwd_cov_gpu.py, from the dense matrices (numpy alone)."""
    H = fc.dense_H(fc.GRIDCOV[gname][0])
    fc.fair(gname, H @ fc.gridcov_dense(gname) @ H.T + fc.NOISE * np.eye(H.shape[0]))


@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("n", [256, 257])
def test_adjoint_and_apply_dev_against_dense_H(gsi, cx, n, with_w):
    indptr, indices, data, lengths = fm.fan(n)
    w = fm.weights(n) if with_w else None
    nobs = len(indptr) - 1
    mdl = gsi.LinearForwardModel((indptr, indices, data, (nobs, n)), weights=w, ctx=cx)
    try:
        assert mdl.adjoint_info() == dict(built=False, resident_bytes=0, long_columns=0, chunks=0, longest_list=0, products=0,
                                          host_products=0)
        info0 = mdl.info()
        V = np.random.default_rng(3).standard_normal((nobs, fm.COLS + 1))
        G = mdl.adjoint(V)
        pl = fm.plan(indptr, indices, data, n, w)
        assert np.array_equal(G, fm.adjoint(pl, V))                       # the host path: the model's bits
        assert np.array_equal(mdl.adjoint(V[:, 0]), G[:, 0])
        H = fm.dense(indptr, indices, data, n, w)
        assert np.abs(G - H.T @ V).max() <= (lengths.max() + 4) * fm.EPS * (np.abs(H).T @ np.abs(V)).max()
        ai = mdl.adjoint_info()
        assert ai["built"] and ai["products"] == 2 and ai["host_products"] == 2, ai
        assert ai["long_columns"] == int((lengths > fm.CHUNK).sum()) and ai["longest_list"] == 3 * fm.CHUNK + 5
        assert ai["chunks"] == len(pl["chunk_off"])
        assert mdl.info()[:5] == info0[:5] and mdl.info()[7] == info0[7]  # gsi_fwd_info does not see the adjoint
        P = np.random.default_rng(4).standard_normal((n, 3))
        Pd = gsi.DeviceMatrix.from_host(cx, P)
        Od = mdl.apply_dev(Pd)
        assert isinstance(Od, gsi.DeviceMatrix) and np.array_equal(Od.to_host(), mdl.apply(P))
        assert np.array_equal(mdl.apply_dev(P), mdl.apply(P)) and mdl.apply_dev(P[:, 0]).shape == (nobs,)
        Od.close()
        Pd.close()
        ref, bound = fwd_cases.reference(indptr, indices, data, n, w, 0, P)
        assert (np.abs(mdl.apply_dev(P) - ref) <= bound).all()
    finally:
        mdl.close()


def test_apply_dev_with_the_exp_link(gsi, cx):
    n = 256
    indptr, indices, data, _ = fm.fan(n)
    mdl = gsi.LinearForwardModel((indptr, indices, data, (len(indptr) - 1, n)), link="exp", ctx=cx)
    try:
        P = 0.5 * np.random.default_rng(4).standard_normal((n, 2))
        assert np.array_equal(mdl.apply_dev(P), mdl.apply(P))
    finally:
        mdl.close()


def test_operator_products(gsi, cx, case, monkeypatch):
    name, Ns, gop, Cm, H = case
    mdl = fc.model(gsi, cx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        assert isinstance(op, gsi.LinearDataOperator)
        fc.products(gsi, op, H @ Cm @ H.T, name, monkeypatch)
    finally:
        op.close()
        mdl.close()


def test_operator_with_weights(gsi, cx, case, monkeypatch):
    name, Ns, gop, Cm, _ = case
    w = fm.weights(int(np.prod(Ns)))
    H = fc.dense_H(Ns, w)
    mdl = fc.model(gsi, cx, Ns, w)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        X = np.random.default_rng(9).standard_normal((H.shape[0], 5))
        fc.close(op.matmul(X), H @ (Cm @ (H.T @ X)), f"{name} weighted")
    finally:
        op.close()
        mdl.close()


def test_solve(gsi, cx, case):
    name, Ns, gop, Cm, H = case
    mdl = fc.model(gsi, cx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        fc.solve_case(gsi, op, H @ Cm @ H.T, name, PATH)
    finally:
        op.close()
        mdl.close()


def test_linear_inversion(gsi, cx, case):
    name, Ns, gop, Cm, H = case
    mdl = fc.model(gsi, cx, Ns)
    try:
        fc.inversion(gsi, gop, mdl, H, Cm, f"linear_inversion {name}")
    finally:
        mdl.close()


def test_condition_on_linear_data(gsi, cx, case):
    name, Ns, gop, Cm, H = case
    mdl = fc.model(gsi, cx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        fc.conditioning(gsi, op, H, Cm, f"conditioning {name}")
    finally:
        op.close()
        mdl.close()


def test_refusals(gsi, cx):
    gop = gsi.fft_powerlaw_operator(cx, [6, 5], -3.5)
    try:
        fc.refusals(gsi, cx, gop, lambda: gsi.Context(0, lib=cx.lib))
    finally:
        gop.close()


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
        gop = gsi.fft_powerlaw_operator(cc, [6, 5], -3.5)
        mdl = fc.model(gsi, cc, (6, 5))
        sc.refused(gsi, lambda: gsi.linear_data_operator(gop, mdl), "communicator")
        mdl.close()
        gop.close()
    finally:
        cc.close()


def test_lifetimes(gsi, cx):
    fc.lifetimes(gsi, cx, lambda: gsi.fft_powerlaw_operator(cx, [6, 5], -3.5), (6, 5))
