"""The bilinear reduction of the likelihood gradient on the GPU: csrc/bilinear_terms.hip through
`gsi_mat_bilinear`, bit for bit against tests/bilinear_model.py and identical from call to call; the same with
GSI_BILINEAR_HOST=1 (the host path of the product library), so device equals host; the refusals.
Cases: tests/bilinear_cases.py."""
import pytest

import bilinear_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()


@pytest.mark.parametrize("n", bc.ROWS)
def test_bits_device(gsi, ctx, n, monkeypatch):
    monkeypatch.delenv("GSI_BILINEAR_HOST", raising=False)
    for b, g in bc.SHAPES:
        bc.run_case(gsi, ctx, n, b, g)


@pytest.mark.parametrize("n", [1, 65, bc.CHUNK + 1, 3 * bc.CHUNK + 5])
def test_bits_host_path(gsi, ctx, n, monkeypatch):
    monkeypatch.setenv("GSI_BILINEAR_HOST", "1")
    for b, g in bc.SHAPES:
        bc.run_case(gsi, ctx, n, b, g)


def test_refusals(gsi, ctx):
    bc.run_refusals(gsi, ctx)
