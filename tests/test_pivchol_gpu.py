"""`gsi_op_pivoted_cholesky` on the device: the kernels of csrc/pivoted_chol.hip (path 1, "fused") under the checks of
tests/pivchol_cases.py -- bit parity with the numpy model at the kernels' loop edges (named there), with the composed leg
(GSI_PCHOL_COMPOSED=1) and with a second call; the stopping rules; every refusal; scattered points against the model on
the operator's own matrix; rank 2048; and what is built on the factor.
PIVCHOL_ERRORS=<path>: the attained figures, as profiles/pivchol_errors.json."""
import json
import os

import numpy as np
import pytest

import pivchol_cases as pv
import pivchol_model as pm

pytestmark = pytest.mark.gpu

PATH = "fused"


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()
    path = os.environ.get("PIVCHOL_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump({"library": "device, fused path", "cases": pv.ERRORS}, f, indent=1, sort_keys=True)
            f.write("\n")


@pytest.mark.parametrize("n,K", pv.DENSE)
def test_parity_dense(gsi, ctx, n, K):
    pv.parity_dense(gsi, ctx, n, K, PATH, also_composed=True)


@pytest.mark.parametrize("nx,ny,K", pv.TABLE + [pv.TABLE_MANY_PARTIALS])
def test_parity_table(gsi, ctx, nx, ny, K):
    pv.parity_table(gsi, ctx, nx, ny, K, PATH, also_composed=True)


def test_parity_gridcov_kinds(gsi, ctx):
    """The other two creators of the implicit grid covariance make the same kind of operator."""
    for kind in (0, 1):
        op = gsi.gridcov_implicit_operator(ctx, 9, 7, 2.5, kind=kind)
        try:
            A = np.asfortranarray(op.matmul(np.eye(63)))
            ref = pm.pivchol(*pm.matrix_source(A), 20)
            pv.check_against_model(f"gridcov kind {kind}", pv.factor(gsi, op, 20), ref, PATH)
        finally:
            op.close()


def test_poll_interval_does_not_change_the_result(gsi, ctx, monkeypatch):
    """Steps enqueued after the stop are no-ops: rank 5 of K = 20 with the state polled after every step, or once."""
    rng = np.random.default_rng(41)
    B = rng.standard_normal((300, 5))
    A = np.asfortranarray(B @ B.T)
    out = []
    for poll in ("1", "64"):
        monkeypatch.setenv("GSI_PCHOL_POLL", poll)
        out.append(gsi.pivoted_cholesky(A, 20, 1e-10, return_info=True, ctx=ctx))
    (L1, p1, r1), (L2, p2, r2) = out
    assert pv.same_bits(L1, L2) and np.array_equal(p1, p2)
    assert (r1["rank"], r1["reason"], r2["rank"], r2["reason"]) == (5, 2, 5, 2)
    assert r1["polls"] == 6 and r2["polls"] == 2, (r1["polls"], r2["polls"])


def test_host_matrix_in_host_factor_out(gsi, ctx):
    pv.host_matrix_in_host_factor_out(gsi, ctx, PATH)


def test_stopping(gsi, ctx):
    pv.stopping(gsi, ctx, PATH)


def test_refusals(gsi, ctx):
    other = gsi.Context(0)
    try:
        pv.refusals(gsi, ctx, other)
    finally:
        other.close()


@pytest.mark.parametrize("kind,d,nugget,seed", pv.SCATTERED)
def test_scattered_points(gsi, ctx, kind, d, nugget, seed):
    pv.scattered(gsi, ctx, kind, d, nugget, seed, PATH)


def test_identities(gsi, ctx):
    pv.identities_dense_table(gsi, ctx, PATH)


def test_large_rank(gsi, ctx):
    pv.large_rank(gsi, ctx, PATH)


def test_preconditioner(gsi, ctx):
    pv.preconditioner(gsi, ctx, PATH)


def test_principal_factor(gsi, ctx):
    pv.principal(gsi, ctx)


@pytest.mark.parametrize("M,N,mu", [(2, 16, 10.0), (8, 64, 0.0), (16, 256, 10.0)])
@pytest.mark.parametrize("principal", [True, False])
def test_getxis_pivchol_feeds_pcgadirect(gsi, ctx, M, N, mu, principal):
    pv.pcga_end_to_end(gsi, ctx, M, N, mu, principal)
