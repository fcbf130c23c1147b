"""Every CholeskyQR kernel instantiation at its dispatch edges, with the tier that ran checked (RandMatFact.jl:57-58, :86).

The thin QR tries three tiers (hip_backend_panels.hip, qr_thinQ): CholeskyQR2, shifted CholeskyQR3, Householder.  A wrong Gram or
triangular-product kernel usually just fails the round-two orthogonality check (cq_orth_check_kernel, 0.1) and the library
moves on to a slower tier that returns a correct Q -- so a test that checks only Q and R does not see it.  Every case here
asserts the counter deltas of a FRESH context (no fall-back hint left by an earlier panel of the same height) as well as
the numbers.

Which kernels a shape reaches (syrk_f64.hip, cholqr.hip):
  Gram matrix G = Y'Y:    sy_kernel<NB, FAST> for 96 <= l <= 320 and m >= 4096, NB = 8 / 10 / 16 / 20 for
                          ceil(l / 16) <= 8 / 10 / 16 / 20; FAST when l == 16 NB and m % 16 == 0.  Otherwise the
                          contraction kernel on the upper tiles (gemm_f64_syrk_upper, tri = 1).
  Cholesky and R^-1:      cq_chol_inv_kernel (one launch) for l <= 384; beyond (or GSI_CQ_FUSED=0) the blocked form:
                          cq_chol_block_kernel per 32 columns plus gemm_f64 with alpha = -1, beta = 1 on sub-views.
  Y R^-1:                 tr_kernel<NB, FAST> for l <= 320 and m >= 4096; FAST for the whole 128-row blocks when
                          l == 16 NB, the general instantiation for a partial last block.  Otherwise the contraction
                          kernel (gemm_f64_trmm_upper, tri = 2).
  Tier gate:              CholeskyQR only for m >= 2 l and l <= 1024.

Reference: Y has integer entries in [-4, 4], so G = Y'Y is exact in fp64 in any summation order (every partial sum is an
integer far below 2^53), and R_ref = chol(G) is computed in long double by the column Cholesky below -- the unique R with
a positive diagonal.  Bound on |R - R_ref| (reference() below): first-order perturbation of the R factor (J.-G. Sun,
"Perturbation bounds for the Cholesky and QR factorizations", BIT 31, 1991) gives ||dR||_F <= sqrt(2) kappa_2(Y) ||dY||_F
for a backward error Y + dY = Q R, and a backward-stable QR of an m x l panel has ||dY||_F <= c l eps ||Y||_2 (inner
products of length l per entry of Q R; the departure of Q from orthonormality, checked separately, adds a term of the same
form).  With c = 1: |R - R_ref|max <= sqrt(2) l eps kappa_2(Y) ||Y||_2.  kappa_2 of these panels lies between ~1.1
(m >> l) and ~6 (m = 2 l).  LAPACK's Householder QR and a host CholeskyQR2 (triangular solves) of the same panels stay 30x
to several 1000x below it.  The bound is not what catches a small kernel error (the 1e-13 bars on Q'Q - I and Y - QR
are); it pins R to the one factor with a positive diagonal, which those bars alone do not.

Out of reach from the Python API: round one's Gram matrix on its own.  CholeskyQR2 corrects a round-one error by design
(round two factors whatever T = Y R1^-1 came out), so a round-one Gram or Cholesky error shows up here only through
round two at the same width (same instantiations) and through the orthogonality check's tier decision; a C ABI hook
to observe it directly is not part of this module.  The contraction kernel's tri = 1 / tri = 2 forms are a run-time
argument, not an instantiation: the shapes that reach them are named in the table.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TIERS = ("cholqr2", "scholqr3", "householder")

# (m, l): the comment names the Gram / Cholesky / Y R^-1 kernels both rounds run
FIRST_TIER = [
    # NB = 8 (l = 128)
    (4096, 128),    # sy<8,FAST>      fused   tr<8,FAST> on every block
    (4112, 128),    # sy<8,FAST>      fused   tr<8,FAST> + tr<8,general> for the 16-row tail block
    (4097, 128),    # sy<8,general>   fused   tr<8,FAST> + tail (m odd; round two: ld = m + 1)
    (4224, 127),    # sy<8,general>   fused   tr<8,general> (ragged last column block)
    (4224, 113),    # sy<8,general>   fused   tr<8,general> (one column in the last block)
    # NB = 10 (l = 160)
    (4096, 160),    # sy<10,FAST>     fused   tr<10,FAST>
    (4144, 160),    # sy<10,FAST>     fused   tr<10,FAST> + tr<10,general> (48-row tail)
    (4099, 160),    # sy<10,general>  fused   tr<10,FAST> + tail
    (4352, 159),    # sy<10,general>  fused   tr<10,general>
    (4352, 145),    # sy<10,general>  fused   tr<10,general>
    # NB = 16 (l = 256)
    (4096, 256),    # sy<16,FAST>     fused   tr<16,FAST>
    (4208, 256),    # sy<16,FAST>     fused   tr<16,FAST> + tr<16,general> (112-row tail)
    (4101, 256),    # sy<16,general>  fused   tr<16,FAST> + tail
    (4096, 255),    # sy<16,general>  fused   tr<16,general>
    (4096, 241),    # sy<16,general>  fused   tr<16,general>
    # NB = 20 (l = 320)
    (4096, 320),    # sy<20,FAST>     fused   tr<20,FAST>
    (4240, 320),    # sy<20,FAST>     fused   tr<20,FAST> + tr<20,general> (16-row tail)
    (4103, 320),    # sy<20,general>  fused   tr<20,FAST> + tail
    (4480, 319),    # sy<20,general>  fused   tr<20,general>
    (4480, 305),    # sy<20,general>  fused   tr<20,general>
    # thresholds
    (4096, 95),     # contraction tri = 1 (l < 96)  fused  tr<8,general>
    (4096, 96),     # sy<8,general> (first width of the dedicated Gram kernel)  fused  tr<8,general>
    (4095, 128),    # m < 4096: contraction tri = 1 and tri = 2  fused
    (640, 320),     # m = 2 l (CholeskyQR gate, open): contraction tri = 1 / tri = 2  fused
    (4096, 321),    # contraction tri = 1 / tri = 2 (l > 320)  fused
    (4096, 384),    # contraction  fused at its largest width (CQF_MAXL)
    (4096, 385),    # contraction  blocked Cholesky (cq_chol_block_kernel + gemm alpha = -1, beta = 1), ragged block
    (2000, 513),    # contraction  blocked, odd l: odd base offsets of the trailing-update sub-views
    (2048, 1024),   # contraction  blocked at the tier's largest width
    # tall: 128 Gram slabs of 560 rows, 35 chunks each
    (70000, 256),   # sy<16,FAST>     fused   tr<16,FAST> + tr<16,general> (112-row tail)
    (70001, 128),   # sy<8,general>   fused   tr<8,FAST> + tail
]
HOUSEHOLDER = [
    (639, 320),     # m = 2 l - 1: CholeskyQR gate closed
    (2050, 1025),   # l > 1024: CholeskyQR gate closed
]
# l = 16 NB: the FAST instantiations, for the runs with a dedicated kernel switched off
FAST_SHAPES = [(4096, 128), (4112, 160), (4096, 256), (4240, 320)]


def int_panel(m, l):
    rng = np.random.default_rng(1000003 * m + l)
    return np.asfortranarray(rng.integers(-4, 5, size=(m, l)).astype(np.float64))


def chol_upper_longdouble(G):
    """Upper Cholesky factor (positive diagonal) of the symmetric positive definite G, column by column in long double."""
    G = np.asarray(G, dtype=np.longdouble)
    l = G.shape[0]
    R = np.zeros((l, l), dtype=np.longdouble)
    for j in range(l):
        c = R[:j, j]
        d = G[j, j] - np.dot(c, c)
        assert d > 0, "Gram matrix not positive definite"
        R[j, j] = np.sqrt(d)
        if j + 1 < l:
            R[j, j + 1:] = (G[j, j + 1:] - np.dot(c, R[:j, j + 1:])) / R[j, j]
    return R


def reference(Y):
    """(R_ref, bound on |R - R_ref|max) for an integer panel Y (module docstring)."""
    l = Y.shape[1]
    G = Y.T @ Y                                   # exact: integer entries, partial sums < 2^53
    assert np.abs(G).max() < 2.0 ** 50
    R_ref = chol_upper_longdouble(G)
    ev = np.linalg.eigvalsh(G)                    # kappa_2(Y)^2 and ||Y||_2^2 (to a few digits: enough for a bound)
    kappa, ynorm = np.sqrt(ev[-1] / ev[0]), np.sqrt(ev[-1])
    return R_ref, np.sqrt(2.0) * l * EPS * kappa * ynorm


def check_qr(Y, Q, R, R_ref, bound, signs_free=False):
    """Q orthonormal and Y = Q R at the bars of test_gpu_parity.test_qr_thinQ; R upper triangular with a positive
    diagonal and within `bound` of R_ref (signs_free: Householder's R, rows compared up to sign)."""
    l = Y.shape[1]
    assert np.abs(Q.T @ Q - np.eye(l)).max() < 1e-13
    assert np.abs(Q @ R - Y).max() < 1e-13 * np.abs(Y).max() * l
    assert np.abs(np.tril(R, -1)).max() == 0.0
    if signs_free:
        R = R * np.where(np.diag(R) < 0, -1.0, 1.0)[:, None]
    assert np.all(np.diag(R) > 0)
    err = float(np.abs(R.astype(np.longdouble) - R_ref).max())
    assert err <= bound, (err, bound)
    return err


def tier_deltas(before, after):
    return {k: after[k] - before[k] for k in TIERS}


def run_qr(gsi, Y):
    """qr_thinQ of Y on a fresh context; (Q, R, counter deltas)."""
    c = gsi.Context(0)
    try:
        before = c.counters()
        Q, R = gsi.qr_thinQ(Y, return_R=True, ctx=c)
        return Q, R, tier_deltas(before, c.counters())
    finally:
        c.close()


# ---- first tier: every instantiation against the long-double reference ---------------------------------------------
@pytest.mark.parametrize("m,l", FIRST_TIER)
def test_cholqr2_first_tier(gsi, m, l):
    Y = int_panel(m, l)
    R_ref, bound = reference(Y)
    Q, R, d = run_qr(gsi, Y)
    assert d == {"cholqr2": 1, "scholqr3": 0, "householder": 0}, (m, l, d)
    check_qr(Y, Q, R, R_ref, bound)


@pytest.mark.parametrize("m,l", HOUSEHOLDER)
def test_cholqr_gate_closed_householder(gsi, m, l):
    Y = int_panel(m, l)
    R_ref, bound = reference(Y)
    Q, R, d = run_qr(gsi, Y)
    assert d == {"cholqr2": 0, "scholqr3": 0, "householder": 1}, (m, l, d)
    check_qr(Y, Q, R, R_ref, bound, signs_free=True)


# ---- second tier at every NB: cond ~ 1e10 panels (as test_gpu_parity.test_qr_paths builds them) ---------------------
# Short panels (m < 64): the shift must clear the Cholesky's own pivot threshold (cholqr.hip, cq_shift_kernel); with
# 4 l sqrt(m) u trace(G) alone these went to Householder.
@pytest.mark.parametrize("m,l", [(4096, 128), (4097, 127), (4096, 160), (4099, 145),
                                 (4096, 256), (4101, 255), (4096, 320), (4103, 305),
                                 (10, 2), (40, 7), (32, 16)])
def test_scholqr3_second_tier(gsi, m, l):
    rng = np.random.default_rng(m + 7 * l)
    U, _ = np.linalg.qr(rng.standard_normal((m, l)))
    V, _ = np.linalg.qr(rng.standard_normal((l, l)))
    Y = np.asfortranarray((U * np.logspace(0, -10, l)) @ V.T)
    Q, R, d = run_qr(gsi, Y)
    assert d == {"cholqr2": 0, "scholqr3": 1, "householder": 0}, (m, l, d)
    assert np.abs(Q.T @ Q - np.eye(l)).max() < 1e-13
    assert np.abs(Q @ R - Y).max() < 1e-13 * l
    assert np.abs(np.tril(R, -1)).max() == 0.0
    s = np.linalg.svd(R, compute_uv=False)
    sref = np.linalg.svd(Y, compute_uv=False)
    assert np.abs(s - sref).max() < 1e-13 * sref[0]


# ---- svd(B) without the thin Q (hip_backend_panels.hip, svd_tall_fused): the same first-tier shapes ---------------------------
@pytest.mark.parametrize("m,l", FIRST_TIER)
def test_svd_tall_fused_first_tier(gsi, m, l):
    W = int_panel(m, l)
    c = gsi.Context(0)
    try:
        before = c.counters()
        S, V = gsi.svd_tall(W, ctx=c)
        d = tier_deltas(before, c.counters())
    finally:
        c.close()
    assert d == {"cholqr2": 1, "scholqr3": 0, "householder": 0}, (m, l, d)
    Sref = np.linalg.svd(W, compute_uv=False)          # dgesdd
    assert np.all(np.diff(S) <= 0)
    assert np.abs(S - Sref).max() <= 1e-12 * Sref[0]
    assert np.abs(V.T @ V - np.eye(l)).max() < 1e-12


# ---- the hint the three first-tier callers share (hip_backend_panels.hip, cholqr2_try / skip_tier1_by_height_) -----------------
def test_first_tier_hint_shared_by_callers(gsi):
    """A failed first tier in svd_tall_fused leaves the hint qr_thinQ reads: eight factorizations of that height start at
    the second tier (the svd_tall's own generic QR is the first of them), the ninth probes from the top again; a panel of
    another height never sees the hint."""
    m, l = 4096, 128
    rng = np.random.default_rng(m + 7 * l)
    U, _ = np.linalg.qr(rng.standard_normal((m, l)))
    V, _ = np.linalg.qr(rng.standard_normal((l, l)))
    W = np.asfortranarray((U * np.logspace(0, -10, l)) @ V.T)         # cond 1e10, as test_scholqr3_second_tier
    Y, Y1 = int_panel(m, l), int_panel(m + 1, l)
    (R_ref, bound), (R1_ref, bound1) = reference(Y), reference(Y1)
    c = gsi.Context(0)
    try:
        def counted(f):
            before = c.counters()
            out = f()
            return out, tier_deltas(before, c.counters())

        def other_height():
            (Q, R), d = counted(lambda: gsi.qr_thinQ(Y1, return_R=True, ctx=c))
            assert d == {"cholqr2": 1, "scholqr3": 0, "householder": 0}, d
            check_qr(Y1, Q, R, R1_ref, bound1)

        other_height()                                                        # before the hint exists
        (S, Vs), d = counted(lambda: gsi.svd_tall(W, ctx=c))
        assert d == {"cholqr2": 0, "scholqr3": 1, "householder": 0}, d        # fused path declined, generic QR one tier down
        Sref = np.linalg.svd(W, compute_uv=False)
        assert np.all(np.diff(S) <= 0)
        assert np.abs(S - Sref).max() <= 1e-12 * Sref[0]
        assert np.abs(Vs.T @ Vs - np.eye(l)).max() < 1e-12
        for i in range(8):
            (Q, R), d = counted(lambda: gsi.qr_thinQ(Y, return_R=True, ctx=c))
            tier = "scholqr3" if i < 7 else "cholqr2"
            assert d == {k: int(k == tier) for k in TIERS}, (i, d)
            check_qr(Y, Q, R, R_ref, bound)
            if i == 3:
                other_height()                                                # while the hint is live
        other_height()                                                        # after it has run out
    finally:
        c.close()


# ---- the same answer with a dedicated kernel switched off (the switches are read once per process: one child each) ---
def child_main(shapes):
    """Runs in a child process: every shape through qr_thinQ on a fresh context, the first-tier checks, one line out."""
    import gsi_amd as gsi
    out = []
    for m, l in shapes:
        Y = int_panel(m, l)
        R_ref, bound = reference(Y)
        Q, R, d = run_qr(gsi, Y)
        assert d == {"cholqr2": 1, "scholqr3": 0, "householder": 0}, (m, l, d)
        out.append([m, l, check_qr(Y, Q, R, R_ref, bound), bound])
    print("forced-ok " + json.dumps(out), flush=True)


CHILD = ("import json, sys\n"
         "sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
         "import test_cholqr_kernels_gpu as t\n"
         "t.child_main(json.loads(sys.argv[3]))\n")


def test_forced_general_paths_same_answer():
    envs = [("general Gram and triangular-product instantiations", {"GSI_SY_NO_FAST": "1", "GSI_TR_NO_FAST": "1"}),
            ("contraction kernel for both", {"GSI_NO_SYRK_KERNEL": "1", "GSI_NO_TRMM_KERNEL": "1"}),
            ("blocked Cholesky", {"GSI_CQ_FUSED": "0"})]
    for what, extra in envs:                          # one after another; the first failure ends the test
        env = dict(os.environ)
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, HERE, json.dumps(FAST_SHAPES)], capture_output=True,
                           text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, (what, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
        lines = [s for s in r.stdout.splitlines() if s.startswith("forced-ok ")]
        assert len(lines) == 1, (what, r.stdout[-2000:])
        assert len(json.loads(lines[0][len("forced-ok "):])) == len(FAST_SHAPES)
