"""The block Jacobi SVD (csrc/jacobi_svd.hip, RandMatFact.jl:86) on every path, to RELATIVE accuracy.

Everything goes through gsi.svd_tall on a fresh gsi.Context(0) per case (no QR tier hint left by an earlier panel picks the
route).  Every case asserts: the sweep cap was not hit (path_info()["svd_sweep_cap_hits"] does not move), at least one sweep
ran, S is descending, S and V are finite.

Graded inputs (jacobi_svd_model.graded): integers -8 .. 8 from a hash, column j scaled by 2^-((7919 j) mod 41), so the column
norms span 2^40 and S[0] / S[-1] ~ 1e12.  The reference is a one-sided Jacobi in long double (jacobi_svd_model.svd_ref; for
the three widest cases its values are committed as tests/golden/jacobi_graded.npz, with a checksum of the regenerated input).
On these inputs dgesdd itself is off by 1e-10 .. 1e-5 relative in the small singular values (measured with the table below),
so it cannot be the reference, and an absolute bar of 1e-12 S[0] does not look at them at all.

Bound: |S_i - ref_i| / ref_i <= l eps kappa_2(W_n), W_n = W with unit columns, kappa computed in the test.  The form is
Demmel and Veselic's for one-sided Jacobi ("Jacobi's method is more accurate than QR", SIAM J. Matrix Anal. Appl. 13, 1992):
the relative error of every singular value is governed by the condition of the column-SCALED matrix, not of W; CholeskyQR2
and Householder QR in front of it are column-wise backward stable, which has the same form.  The constant is 1 (as in
test_cholqr_kernels_gpu.py).  The float64 model of the same scheme (jacobi_svd_model.svd_model on cholqr2_R / numpy's QR)
sits at this fraction of the bound, asserted <= 0.25 by tests/test_jacobi_svd_model.py for every case before the bound is
used here:

  (n, l)       kappa_2(W_n)  model / bound   dgesdd rel. error      (n, l)        kappa_2(W_n)  model / bound   dgesdd
  (8, 1)        1.00          0.155           1e-16                 (330, 160)     5.19          0.137           3e-06
  (8, 2)        3.10          0.115           3e-17                 (360, 176)     5.49          0.129           6e-06
  (40, 16)      3.05          0.207           4e-10                 (330, 161)     5.24          0.137           1e-06
  (40, 17)      3.07          0.218           1e-10                 (520, 256)     5.39          0.139           9e-06
  (70, 31)      4.35          0.142           2e-08                 (650, 320)     5.50          0.147           4e-06
  (70, 32)      4.43          0.147           2e-08                 (1210, 601)    5.48          0.159           1e-05
  (70, 33)      4.76          0.164           7e-09                 Householder route (n < 2 l):
  (100, 48)     4.76          0.131           6e-08                 (50, 33)       6.48          0.093           9e-09
                                                                    (130, 96)     12.03          0.058           5e-07
                                                                    (200, 160)    18.61          0.040           2e-06
  forced widths 8 / 4 / 2, l in {1, 2, 15, 16, 17, 40, 41, 96} at n = 2 l + 4: model / bound between 0.01 and 0.25.

Which tier hands R to the Jacobi kernel is the QR gate's decision (hip_backend_panels.hip, qr_thinQ), not the test's: n >= 2 l only
ADMITS a panel to the Cholesky tiers.  Their guards look at the UNSCALED panel, so a column grading of 2^40 fails
CholeskyQR2's although CholeskyQR2 on such a panel would be accurate (Cholesky is invariant under column scaling; the
float64 model above is exactly that chain).  Every case asserts the relative bound on whichever tier ran, except the shifted
tier, whose shift is an absolute perturbation: there the absolute bar 1e-12 S[0] is asserted and a warning says so.  Seen on
an MI355X (device error / bound; the shifted-tier ratios are what the relative bound would have seen):

  (8, 1) 0.155 and (8, 2) 0.019: CholeskyQR2.
  (40, 16) 0.143, (40, 17) 0.162, (70, 31) 0.107, (70, 32) 0.100, (70, 33) 0.095, (100, 48) 0.101: shifted CholeskyQR3.
  (330, 160) 0.105, (360, 176) 0.087, (330, 161) 0.102, (520, 256) 0.099, (650, 320) 0.110, (1210, 601) 0.112: both
    Cholesky tiers refuse, Householder runs.
  (50, 33) 0.087, (130, 96) 0.043, (200, 160) 0.030: Householder (n < 2 l).
  scaled by 2^+-120: (70, 33) 0.095 shifted, (330, 160) 0.105 Householder -- the unscaled figures to every digit printed.
  forced widths 8 / 4 / 2: 0.019 .. 0.161 for l >= 2, 0.600 for l = 1 (bound = eps: one rounding of the norm's sqrt).
So the graded inputs reach the Jacobi kernel behind the CholeskyQR2 tier only at l <= 2; the finding is about the gate.

Limits of the rotation test.  c*c > tol2 * (a*b) is evaluated as written, with a, b <= l max|R|^2: a*b overflows for
|R| > ~2^255 / sqrt(l) (then inf > inf is false and nothing rotates), and c*c or tol2 * (a*b) (tol2 ~ 2^-100) lose bits
to the subnormal range for |R| < ~2^-255, where the test starts to misjudge.  The scaled cases (W 2^120 and W 2^-120:
(l 2^240)^2 and tol2 2^-480 are far inside the fp64 range) show that the result is scale-invariant well inside these
limits; nothing is tested beyond them.  DESIGN.md section 4.4 states the same.
"""
import functools
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np
import pytest

import jacobi_svd_model as jm
from helpers import exact_rank_matrix

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TIERS = ("cholqr2", "scholqr3", "householder")
GOLDEN = os.path.join(HERE, "golden", "jacobi_graded.npz")

# (n, l, what the width reaches in svd_small -- the keys are those of jacobi_svd_model.dispatch, and
# tests/test_jacobi_svd_model.py asserts that dispatch(l) agrees, so the table cannot drift from the code)
GRADED_CHOLQR = [
    (8, 1, {"svd_w": 16, "nblk": 2, "activity": False}),                       # one column
    (8, 2, {"svd_w": 16, "nblk": 2, "activity": False}),
    (40, 16, {"svd_w": 16, "nblk": 2, "activity": False}),                     # block 1 all padding
    (40, 17, {"svd_w": 16, "nblk": 2, "activity": False}),
    (70, 31, {"svd_w": 16, "nblk": 2, "activity": False}),
    (70, 32, {"svd_w": 16, "nblk": 2, "activity": False, "ni": 0}),            # single workgroup, full blocks
    (70, 33, {"svd_w": 16, "nblk": 4, "activity": True, "first_look": 1}),     # padding block; activity-driven from sweep 1
    (100, 48, {"svd_w": 16, "nblk": 4, "activity": True, "first_look": 1}),
    (330, 160, {"svd_w": 16, "nblk": 10, "ni": 10, "resident": True, "activity": True, "first_look": 4}),   # NI = 10
    (360, 176, {"svd_w": 16, "nblk": 12, "ni": 0, "resident": False, "activity": True}),   # multiple of 16, generic NI = 0
    (330, 161, {"svd_w": 16, "nblk": 12, "ni": 0, "resident": False, "activity": True}),   # odd l: scalar loads and stores
    (520, 256, {"svd_w": 16, "nblk": 16, "ni": 16, "resident": True, "activity": True}),   # NI = 16, golden
    (650, 320, {"svd_w": 16, "nblk": 20, "ni": 20, "resident": True, "activity": True}),   # NI = 20, golden
    (1210, 601, {"svd_w": 8, "nblk": 76, "ni": 0, "resident": False, "activity": False}),  # <8>, odd l, golden
]
GRADED_HOUSEHOLDER = [
    (50, 33, {"svd_w": 16, "nblk": 4, "activity": True}),
    (130, 96, {"svd_w": 16, "nblk": 6, "activity": True}),
    (200, 160, {"svd_w": 16, "nblk": 10, "ni": 10, "resident": True, "activity": True}),
]
SCALED = [(70, 33), (330, 160)]
# instantiations and LDS limits at the suite's own bars; lds_bytes of a 163,776 B request
LIMITS = [
    (1200, 600, {"svd_w": 16, "nblk": 38, "lds_bytes": 159760, "activity": True}),     # widest 16-column blocking
    (1210, 601, {"svd_w": 8, "nblk": 76, "lds_bytes": 79888}),                         # first width of <8>
    (1220, 608, {"svd_w": 8, "nblk": 76, "ni": 0}),                                    # multiple of 16 under <8>: generic
    (1200, 1200, {"svd_w": 8, "nblk": 150, "lds_bytes": 153616}),                      # widest <8>; Householder (l > 1024)
    (1201, 1201, {"svd_w": 4, "nblk": 302, "lds_bytes": 78864}),                       # first width of <4>, odd
    (2500, 2500, {"svd_w": 4, "nblk": 626, "lds_bytes": 160784}),                      # widest <4>
]
FORCED_WIDTHS = (8, 4, 2)
FORCED_L = (1, 2, 15, 16, 17, 40, 41, 96)                                              # at n = 2 l + 4
# hash seeds other than 0.  (6, 1): with seed 0 the float64 model used 0.335 of the bound (one column: the bound is eps, and
# sqrt(82) rounds badly); with seed 7 it uses 0.009.
SEEDS = {(6, 1): 7}
# the sparse schedule by construction: (l, blocks of 16 columns made dense, what the schedule builder has to do)
SPARSE = [
    (96, (0, 3), "one edge, both diagonals"),
    (96, (2,), "a block active only within itself: the partner branch"),
    (40, (2,), "block 2 holds 8 columns, its partner is the all-padding block 3"),
    (112, (0, 1, 2), "three edges, three rounds"),
]


# ---- running one case -------------------------------------------------------------------------------------------------------
def run_svd(gsi, W):
    """svd_tall of W on a fresh context with the assertions every case makes; (S, V, info)."""
    c = gsi.Context(0)
    try:
        before, cap0 = c.counters(), c.path_info()["svd_sweep_cap_hits"]
        t0 = time.perf_counter()
        S, V = gsi.svd_tall(W, ctx=c)
        seconds = time.perf_counter() - t0
        after, cap1 = c.counters(), c.path_info()["svd_sweep_cap_hits"]
    finally:
        c.close()
    info = {k: after[k] - before[k] for k in TIERS}
    info["sweeps"] = after["jacobi_sweeps"]
    info["seconds"] = seconds
    assert cap1 == cap0, ("the sweep cap was hit", W.shape, info)
    assert info["sweeps"] >= 1, info
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(V)), W.shape
    assert np.all(np.diff(S) <= 0), ("S is not descending", W.shape)
    return S, V, info


@functools.lru_cache(maxsize=None)
def graded_case(n, l):
    """(W, long-double reference, bound) of a graded case; the three widest references come from the golden file, after
    the regenerated input passed its checksum."""
    W = jm.graded(n, l, seed=SEEDS.get((n, l), 0))
    W.setflags(write=False)
    with np.load(GOLDEN) as g:
        if f"S_{n}_{l}" in g:
            assert jm.exact_sum(W) == float(g[f"sum_{n}_{l}"]), "the regenerated input is not the one the golden file was made from"
            ref = g[f"S_{n}_{l}"].astype(np.longdouble)
        else:
            ref = jm.svd_ref(W)
    ref.setflags(write=False)
    return W, ref, jm.relative_bound(W)


def check_relative(S, ref, bound, info, scale=1.0):
    """The relative bound, whichever tier produced R -- except where the SHIFTED CholeskyQR3 tier ran (its shift perturbs
    every singular value by ~ l sqrt(n) eps S[0]): there the suite's absolute bar, with a message that says so."""
    assert info["cholqr2"] + info["scholqr3"] + info["householder"] == 1, info
    ref = ref * np.longdouble(scale)
    rel = float(np.max(np.abs(S.astype(np.longdouble) - ref) / ref))
    print(f"  max rel. error {rel:.3e}, bound {bound:.3e} (ratio {rel / bound:.3f}); tiers {[info[k] for k in TIERS]}, "
          f"{info['sweeps']} sweeps, {info['seconds']:.2f} s")
    if info["scholqr3"]:
        err = float(np.max(np.abs(S.astype(np.longdouble) - ref)))
        msg = (f"the SHIFTED CholeskyQR3 tier ran for this graded input (tier gate), so only the absolute bar 1e-12 S[0] is "
               f"asserted, not the relative bound: rel. error {rel:.3e}, bound {bound:.3e}")
        warnings.warn(msg)
        assert err <= 1e-12 * float(ref[0]), (msg, err, float(ref[0]))
        return
    assert rel <= bound, (rel, bound, info)


def check_bars(W, S, V, Sref=None):
    """The suite's own bars (test_gpu_parity.test_svd_tall_clustered_spectrum)."""
    l = W.shape[1]
    if Sref is None:
        Sref = np.linalg.svd(W, compute_uv=False)             # dgesdd
    assert np.abs(S - Sref).max() <= 1e-12 * Sref[0]
    assert np.abs(V.T @ V - np.eye(l)).max() < 1e-11
    R = V.T @ W                                               # rows of V'W have norms S
    assert np.linalg.norm(W - V @ R) <= 1e-11 * np.linalg.norm(W)
    assert np.abs(np.linalg.norm(R, axis=1) - S).max() <= 1e-11 * S[0]


# ---- 3a. relative accuracy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,l", [(n, l) for n, l, _ in GRADED_CHOLQR])
def test_graded_relative_accuracy_cholqr_route(gsi, n, l):
    """n >= 2 l: the panel is offered to CholeskyQR2 first; the tier that accepts it is printed (module docstring)."""
    W, ref, bound = graded_case(n, l)
    S, V, info = run_svd(gsi, W)
    check_relative(S, ref, bound, info)
    assert np.abs(V.T @ V - np.eye(l)).max() < 1e-11


@pytest.mark.parametrize("n,l", [(n, l) for n, l, _ in GRADED_HOUSEHOLDER])
def test_graded_relative_accuracy_householder_route(gsi, n, l):
    """n < 2 l: Householder hands R to the Jacobi kernel -- no Gram matrix in front of it."""
    W, ref, bound = graded_case(n, l)
    S, V, info = run_svd(gsi, W)
    assert (info["cholqr2"], info["scholqr3"], info["householder"]) == (0, 0, 1), info
    check_relative(S, ref, bound, info)
    assert np.abs(V.T @ V - np.eye(l)).max() < 1e-11


@pytest.mark.parametrize("n,l", SCALED)
@pytest.mark.parametrize("bits", [120, -120])
def test_graded_scaled_inputs(gsi, n, l, bits):
    """W 2^120 and W 2^-120 against ref 2^+-120 with the same bound: a b and c c stay normal numbers (module docstring)."""
    W, ref, bound = graded_case(n, l)
    scale = float(np.ldexp(1.0, bits))
    S, V, info = run_svd(gsi, np.asfortranarray(W * scale))
    check_relative(S, ref, bound, info, scale=scale)


# ---- 3b. instantiations and limits at the suite's bars ---------------------------------------------------------------------
def logspace_input(n, l):
    return np.asfortranarray(jm.hashed_ints(n, l, seed=3) * np.logspace(0, -3, l)[None, :])


@pytest.mark.parametrize("n,l", [(n, l) for n, l, _ in LIMITS])
def test_instantiations_and_lds_limits(gsi, n, l):
    W = logspace_input(n, l)
    S, V, info = run_svd(gsi, W)
    print(f"  ({n}, {l}): tiers {[info[k] for k in TIERS]}, {info['sweeps']} sweeps, svd_tall took {info['seconds']:.2f} s")
    assert info["householder"] == (1 if l > 1024 else 0), info
    check_bars(W, S, V)


def child_main(width):
    """In a child process with GSI_SVD_W = width: the graded cases FORCED_L at n = 2 l + 4, the relative bound, one line out."""
    import gsi_amd as gsi
    assert int(os.environ["GSI_SVD_W"]) == width
    out = []
    for l in FORCED_L:
        assert jm.dispatch(l, width)["svd_w"] == width
        n = 2 * l + 4
        W, ref, bound = graded_case(n, l)
        S, V, info = run_svd(gsi, W)
        check_relative(S, ref, bound, info)
        assert np.abs(V.T @ V - np.eye(l)).max() < 1e-11
        out.append([n, l, float(np.max(np.abs(S.astype(np.longdouble) - ref) / ref)), bound, info["sweeps"]])
    print("forced-ok " + json.dumps(out), flush=True)


CHILD = ("import sys\n"
         "sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
         "import test_jacobi_svd_gpu as t\n"
         "t.child_main(int(sys.argv[3]))\n")


def test_forced_block_widths():
    """jacobi_block_kernel<8>, <4> and <2> on small widths (GSI_SVD_W is read once per process: one child per width, one after
    another; the first failure ends the test and starts no further child)."""
    for width in FORCED_WIDTHS:
        env = dict(os.environ)
        env["GSI_SVD_W"] = str(width)
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, HERE, str(width)], capture_output=True, text=True,
                           timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, (width, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
        lines = [s for s in r.stdout.splitlines() if s.startswith("forced-ok ")]
        assert len(lines) == 1, (width, r.stdout[-2000:])
        got = json.loads(lines[0][len("forced-ok "):])
        assert [g[1] for g in got] == list(FORCED_L)
        print(f"  width {width}: " + ", ".join(f"l={g[1]} {g[2] / g[3]:.3f}" for g in got))


# ---- 3c. exact and edge inputs ---------------------------------------------------------------------------------------------
def diagonal_input(l):
    """W = [diag(d); 0], d_j = 2^-((7919 j) mod 13): powers of two, unsorted, every value several times."""
    d = np.ldexp(1.0, -((7919 * np.arange(l)) % 13))
    W = np.zeros((2 * l, l), order="F")
    W[np.arange(l), np.arange(l)] = d
    return W, d


@pytest.mark.parametrize("l", [33, 160, 600])
def test_diagonal_input_is_exact(gsi, l):
    """Gram matrix (sums of one product and zeros), Cholesky (square roots of even powers of two), inverse and triangular
    products are exact here, so R = diag(d) exactly; no pair rotates; the norms are exact.  S must be the sorted d bit for bit
    and V exactly the permutation that ranks equal values lower column first (jacobi_finish_kernel's stable order)."""
    W, d = diagonal_input(l)
    S, V, info = run_svd(gsi, W)
    assert (info["cholqr2"], info["scholqr3"], info["householder"]) == (1, 0, 0), info
    order = np.argsort(-d, kind="stable")                     # order[rank] = column: descending, ties lower column first
    assert np.array_equal(S, d[order])
    P = np.zeros((2 * l, l))
    P[order, np.arange(l)] = 1.0
    assert np.array_equal(V, P)
    if l < 128:
        assert info["sweeps"] == 1, info                      # (from 128 columns on the first look comes after sweep 4)


@pytest.mark.parametrize("n,l,col", [(50, 33, 7), (70, 17, 16), (40, 40, 33)])
def test_zero_column(gsi, n, l, col):
    """A literally zero column (the a > 0 && b > 0 guard of the rotation, the zero-norm branch of jacobi_finish_kernel)."""
    W = np.array(logspace_input(n, l), order="F")
    W[:, col] = 0.0
    S, V, info = run_svd(gsi, W)
    print(f"  ({n}, {l}): tiers {[info[k] for k in TIERS]}, {info['sweeps']} sweeps")
    Sref = np.linalg.svd(W, compute_uv=False)
    assert S[-1] == 0.0
    assert np.abs(S - Sref).max() <= 1e-12 * Sref[0]
    assert np.abs(V[:, :l - 1].T @ V[:, :l - 1] - np.eye(l - 1)).max() < 1e-11


@pytest.mark.parametrize("n,l,j1,j2", [(50, 33, 3, 20), (70, 17, 0, 16), (200, 160, 5, 150)])
def test_two_identical_columns(gsi, n, l, j1, j2):
    """Columns j1 and j2 equal: their images in R have the same norm (to the last bit or two), so the pair's first rotation
    is the d = b - a = 0 one, t = +-1."""
    W = np.array(logspace_input(n, l), order="F")
    W[:, j2] = W[:, j1]
    S, V, info = run_svd(gsi, W)
    print(f"  ({n}, {l}): tiers {[info[k] for k in TIERS]}, {info['sweeps']} sweeps")
    Sref = np.linalg.svd(W, compute_uv=False)
    assert np.abs(S - Sref).max() <= 1e-12 * Sref[0]


@pytest.mark.parametrize("n,l,r", [(300, 48, 20), (400, 160, 37)])
def test_exact_rank(gsi, n, l, r):
    """makeA-style exact rank r < l: the leading r values and vectors at the suite's bars, the rest at rounding level.
    Seen on the device (not asserted): the trailing l - r columns of V are unit vectors, orthogonal to the leading ones to
    ~1e-15 and among themselves to ~1e-5 (they are R's rounding noise normalised, rotated only down to tol relative to
    each other) -- see the printed figures."""
    rng = np.random.default_rng(1000 * n + l)
    W = np.asfortranarray(exact_rank_matrix(rng, n, r)[:, :l])
    S, V, info = run_svd(gsi, W)
    Sref = np.linalg.svd(W, compute_uv=False)
    assert np.abs(S[:r] - Sref[:r]).max() <= 1e-12 * Sref[0]
    assert np.all(S[r:] <= 1e-12 * Sref[0])
    Vr = V[:, :r]
    assert np.abs(Vr.T @ Vr - np.eye(r)).max() < 1e-11
    R = Vr.T @ W
    assert np.linalg.norm(W - Vr @ R) <= 1e-11 * np.linalg.norm(W)
    assert np.abs(np.linalg.norm(R, axis=1) - S[:r]).max() <= 1e-11 * S[0]
    Vt = V[:, r:]
    print(f"  ({n}, {l}, rank {r}): tiers {[info[k] for k in TIERS]}, {info['sweeps']} sweeps; trailing columns of V: norms "
          f"{np.linalg.norm(Vt, axis=0).min():.3e} .. {np.linalg.norm(Vt, axis=0).max():.3e}, |Vt'Vt - I|max "
          f"{np.abs(Vt.T @ Vt - np.eye(l - r)).max():.3e}, |Vr'Vt|max {np.abs(Vr.T @ Vt).max():.3e}")


# ---- 3d. the sparse schedule, reached by construction ----------------------------------------------------------------------
def sparse_input(l, blocks):
    """W = [T; 0] (2 l x l): T diagonal with the distinct powers of two 2^-((37 j) mod l), and for every column of the 16-column
    blocks `blocks` hash entries added in the rows of those blocks only.  A column outside the set is a multiple of a unit
    vector whose row no other column touches: its Gram entries, its row and column of the Cholesky factors and of R are exact
    zeros off the diagonal, so it never couples with anything, and after the first sweep only the set's block pairs are
    flagged."""
    assert np.gcd(37, l) == 1
    W = np.zeros((2 * l, l), order="F")
    W[np.arange(l), np.arange(l)] = np.ldexp(1.0, -((37 * np.arange(l)) % l))
    idx = np.concatenate([np.arange(16 * b, min(16 * b + 16, l)) for b in blocks])
    W[np.ix_(idx, idx)] += jm.hashed_ints(len(idx), len(idx), seed=5)
    return W


@pytest.mark.parametrize("l,blocks", [(l, b) for l, b, _ in SPARSE])
def test_sparse_schedule_by_construction(gsi, l, blocks):
    """Only the dense set's block pairs are active after the first look (2 active <= npairs: sparse sweeps from the second
    on), and the dense set cannot converge in two sweeps (tests/test_jacobi_svd_model.py shows the model still active after
    its second), so at least the second and third sweeps run on a host-built schedule."""
    W = sparse_input(l, blocks)
    d = jm.dispatch(l)
    assert d["activity"] and d["first_look"] == 1
    nact = len(blocks) * (len(blocks) + 1) // 2
    assert 2 * nact <= d["nblk"] * (d["nblk"] + 1) // 2
    S, V, info = run_svd(gsi, W)
    print(f"  l = {l}, dense blocks {blocks}: tiers {[info[k] for k in TIERS]}, {info['sweeps']} sweeps")
    assert info["sweeps"] >= 3, info
    check_bars(W, S, V)
