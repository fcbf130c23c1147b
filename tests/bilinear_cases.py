"""The cases of the bilinear reduction (`gsi_mat_bilinear`), run by tests/test_bilinear_cpu.py on the
CPU reference library (csrc/bilinear_terms_host.hpp) and by tests/test_bilinear_gpu.py on the device kernel and, with
GSI_BILINEAR_HOST=1, on the host path of the product library.  Every result must equal tests/bilinear_model.py bit for bit."""
import numpy as np

import bilinear_model as bm
import solve_cases as sc

CHUNK = bm.CHUNK
# the row counts at which the code takes another path: one row, one tile of 64 and its neighbours, a chunk and its
# neighbours, several chunks with a ragged end (odd)
ROWS = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
# (b, g): one column alone, g = 0, g = b, g = 16 = b, g = 16 with probe columns beyond one group of 32, g below 16
SHAPES = [(1, 0), (1, 1), (5, 0), (4, 4), (16, 16), (16 + 33, 16), (7, 3), (40, 2)]


def operands(n, b, seed):
    rng = np.random.default_rng([seed, n, b])
    # magnitudes spread over several binades, so that another order of additions gives other bits
    scale = lambda: np.exp2(rng.integers(-6, 7, size=(n, b)).astype(np.float64))
    return rng.standard_normal((n, b)) * scale(), rng.standard_normal((n, b)) * scale(), rng.standard_normal((n, b)), rng.standard_normal(n)


def run_case(gsi, ctx, n, b, g, seed=1):
    """All four operand forms (dd and R, R without dd, neither) at one shape, two calls each."""
    Lh, Yh, Rh, dd = operands(n, b, seed)
    Ld, Yd, Rd = (gsi.DeviceMatrix.from_host(ctx, a) for a in (Lh, Yh, Rh))
    try:
        for use_dd, use_R in ((True, True), (False, True), (False, False)):
            want_g, want_t = bm.terms(Lh, Yh, Rh if use_dd else None, dd if use_dd else None, g)
            for _ in range(2):                                  # two calls return the same bits
                got_g, got_t = gsi.mat_bilinear(Ld, Yd, Rd if use_R else None, dd if use_dd else None, g)
                assert got_g.shape == (g, g) and got_t.shape == (b - g,)
                assert np.array_equal(got_g, want_g), (n, b, g, use_dd, np.abs(got_g - want_g).max())
                assert np.array_equal(got_t, want_t), (n, b, g, use_dd, np.abs(got_t - want_t).max())
        for d, h in ((Ld, Lh), (Yd, Yh), (Rd, Rh)):             # the panels are not written
            assert np.array_equal(d.to_host(), h)
    finally:
        for d in (Ld, Yd, Rd):
            d.close()


def run_model_is_ordered():
    """The model itself: a case where pairwise or fused evaluation gives other bits than the stated order."""
    L = np.array([[1.0 + 2.0 ** -30], [1.0], [1.0]])
    Y = np.array([[1.0 - 2.0 ** -30], [2.0 ** -53], [2.0 ** -53]])
    gram, t = bm.terms(L, Y, g=1)
    # fl((1 + e)(1 - e)) = 1; then 2^-53 twice, one at a time: both are lost
    assert gram[0, 0] == 1.0 and t.size == 0
    _, t = bm.terms(np.hstack([L, L]), np.hstack([Y, Y]), g=0)
    assert np.array_equal(t, [1.0, 1.0])
    # dd .* R is rounded before it is added
    g2, _ = bm.terms(np.ones((1, 1)), np.array([[1.0]]), np.array([[1.0 + 2.0 ** -30]]), np.array([1.0 - 2.0 ** -30]), g=1)
    assert g2[0, 0] == 2.0


def run_refusals(gsi, ctx):
    A, B, Cw = gsi.DeviceMatrix(ctx, 5, 20), gsi.DeviceMatrix(ctx, 5, 20), gsi.DeviceMatrix(ctx, 5, 19)
    try:
        sc.refused(gsi, lambda: gsi.mat_bilinear(A, B, None, None, 17), "min(b, 16)")
        sc.refused(gsi, lambda: gsi.mat_bilinear(A, B, None, None, -1), "min(b, 16)")
        sc.refused(gsi, lambda: gsi.mat_bilinear(Cw, Cw, None, None, 20), "min(b, 16)")       # g > b
        sc.refused(gsi, lambda: gsi.mat_bilinear(A, Cw, None, None, 2), "shape of L")
        sc.refused(gsi, lambda: gsi.mat_bilinear(A, B, Cw, None, 2), "shape of L")
        sc.refused(gsi, lambda: gsi.mat_bilinear(A, B, None, np.ones(5), 2), "dd needs R")
        sc.refused(gsi, lambda: gsi.mat_bilinear(A, B, B, np.array([1.0, np.nan, 1.0, 1.0, 1.0]), 2), "non-finite")
        with np.testing.assert_raises(ValueError):
            gsi.mat_bilinear(A, B, B, np.ones(4), 2)
    finally:
        for d in (A, B, Cw):
            d.close()
