"""gemm_f64_kernel<NT, TRANS_A, 0, XMODE> (csrc/gemm_f64_kernel.inc.hpp), its launcher and splitk_reduce_kernel
(csrc/gemm_f64.hip), instantiation by instantiation, through the views the library's own callers pass: leading dimensions
larger than the rows, 8-byte-aligned bases, beta != 0, the triangular forms and the row blocks.

Every case goes through gsi_gemm_view: the operands lie where the case says inside allocations filled with NaN, C travels
as its whole image, and the call reports what the LAUNCHER decided (tiles per chunk, chunks, XMODE, 16-byte loads, K
splits, persistent mode), so the assertions are about the instantiation that ran.  tests/gemm_cases.py holds the table, the
references and the checks; tests/test_gemm_cases.py runs the same checks on the CPU against a numpy stand-in.

Per case:  exact   np.array_equal with the int64 product on the view; every double of the image outside the view bit-equal
                   to what was uploaded; beta == 0 starts from an all-NaN C and must end finite;
           real    |C - ref| <= gamma_(K+2) (|alpha||A||B| + |beta||C0|) entry by entry against np.longdouble;
           plan    the fields the table expects (NT, chunks, XMODE, wide, splits, persistent).
tri = 1 is checked on row <= col only; tri = 2 (B upper triangular, zeros below) must also match form 0 bit for bit; the
row blocks of form 3 put together must match form 0 bit for bit.

test_table_reaches_every_path is a condition on the table: the union of the reported plans holds every (NT, TRANS) under
XMODE 0 and XMODE 1, XMODE 2 for NN and TN, both load widths, split counts that are and are not multiples of 8 (the two
workgroup-to-split mappings), the persistent mode, 1 to 3 column chunks and the forms 1 to 3.

The largest error / bound ratio of each real case: profiles/gemm_kernel_errors.json, written by a run with
GSI_GEMM_RECORD=<path>.  Measured on the MI355X: every case passes; the largest ratio is 0.148 (K = 33, the persistent
mode's row count), the split products stay below 0.001; the module takes 8.4 s, of which the persistent group's 84 MB C
images are 4.1 s and the six large-leading-dimension cases 0.05 s.

That the table sees what it claims was checked once on the device with two perturbed builds of gemm_f64.hip (not kept):
splitk_reduce_kernel reading C under beta == 0 failed exactly the split cases that start from a NaN C (4 of group split, the
5 split cases of tri1, the 8 of tri2 and all four row-block tests) and passed the rest; the launcher counting one tile too
few per row block of the symmetric product failed exactly the two tri1 cases with more than one row block (l = 320, 384).
"""
import functools
import json
import os
import time

import numpy as np
import pytest

import gemm_cases as gc

pytestmark = pytest.mark.gpu

RECORD_ENV = "GSI_GEMM_RECORD"
_runs = {}          # group -> {case id: (case, plan, failures, ratio)}
_walls = {}
_device_error = []  # the first exception out of the library: after it nothing more is launched in this process


def _view(gsi, ctx):
    def call(*a, **kw):
        if _device_error:
            pytest.fail("not launched: an earlier call failed with " + _device_error[0])
        try:
            return gsi.gemm_view(*a, ctx=ctx, **kw)
        except Exception as e:
            _device_error.append(repr(e))
            raise
    return call


def _run_group(gsi, group):
    if group in _runs:
        return _runs[group]
    ctx = gsi.default_context()
    t0 = time.perf_counter()
    out = {}
    for case in gc.group_cases(group):
        img0, img, plan, ops = gc.run_case(_view(gsi, ctx), case)
        bad, ratio = gc.check_case(case, img0, img, plan, ops)
        print("%s plan=%s%s%s" % (case.id, [plan[f] for f in gc.PLAN_FIELDS], "" if ratio is None else " ratio=%.4f" % ratio,
                                  (" FAILED: " + "; ".join(bad)) if bad else ""))
        out[case.id] = (case, plan, bad, ratio, img)
    if group == "tri2":                     # form 2 against form 0 on the same operands
        by = {c.id: v for c, *v in out.values()}
        for cid, (case, plan, bad, ratio, img) in out.items():
            if case.form == 2:
                twin = gc.replace(case, form=0)
                if not gc._same_bits(gc.view_of(case, img), gc.view_of(twin, by[twin.id][3])):
                    bad.append("form 2 and form 0 differ in bits")
    out = {cid: v[:4] for cid, v in out.items()}
    if group in gc.BIG_GROUPS:
        ctx.release_cache()             # GBs of exact-size blocks nobody else will ask for
    _walls[group] = time.perf_counter() - t0
    _runs[group] = out
    return out


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    path = os.environ.get(RECORD_ENV)
    if path and _runs:
        cases = [{"case": cid, "K": c.k, "ratio": r} for g in _runs.values() for cid, (c, _, _, r) in g.items() if r is not None]
        cases += [{"case": k, "bit_identical_to_form_0": v} for k, v in _rowblock_record.items()]
        with open(path, "w") as f:
            json.dump({"bound": "gamma_(K+2) (|alpha| |A||B| + |beta| |C0|) per entry against np.longdouble, gamma_n = n u / (1 - n u), u = 2^-53",
                       "largest_ratio": max([c["ratio"] for c in cases if "ratio" in c], default=None),
                       "exact_cases": sum(1 for g in _runs.values() for (c, _, _, _) in g.values() if not c.real),
                       "cases": cases}, f, indent=1)
            f.write("\n")


@pytest.mark.parametrize("group", list(gc.GROUPS))
def test_group(gsi, group):
    out = _run_group(gsi, group)
    failed = {cid: bad for cid, (_, _, bad, _) in out.items() if bad}
    assert not failed, "%d of %d cases failed:\n%s" % (len(failed), len(out), "\n".join("%s: %s" % kv for kv in failed.items()))


_rowblock_record = {}
_rowblock_runs = {}


@functools.lru_cache(maxsize=None)
def _rowblock_operands(shape):
    m_full, k, l = shape
    rng = np.random.default_rng(m_full + k)
    A, B = np.asfortranarray(rng.standard_normal((m_full, k))), np.asfortranarray(rng.standard_normal((k, l)))
    ld_ = np.longdouble
    return A, B, gc.matmul_rows(A.astype(ld_), B.astype(ld_)), gc.gamma(k + 2) * gc.matmul_rows(np.abs(A).astype(ld_), np.abs(B).astype(ld_))


def _run_rowblocks(gsi, shape, cuts):
    """-> list of failures; the blocks' plans join the table's."""
    if (shape, cuts) in _rowblock_runs:
        return _rowblock_runs[(shape, cuts)]
    m_full, k, l = shape
    ctx = gsi.default_context()
    A, B, ref_ld, bound = _rowblock_operands(shape)
    whole = gc.Case(group="rowblock", m=m_full, l=l, k=k, real=True, lda=gc.ld(m_full, 0), ldb=gc.ld(k, 0), ldc=gc.ld(m_full, 0), c_off=2)
    img0 = np.full(whole.image_doubles, np.nan)
    kw = dict(l=l, k=k, lda=whole.LDA, ldb=whole.LDB, ldc=whole.LDC, c_off=whole.c_off)
    view = _view(gsi, ctx)
    bad = []
    ref_img, ref_plan = view(A, B, img0, m=m_full, form=0, **kw)
    if ref_plan["nsplit"] <= 1:
        bad.append("the whole product is not split")
    ref = gc.view_of(whole, ref_img)
    if not (np.isfinite(ref).all() and (np.abs(ref.astype(np.longdouble) - ref_ld) <= bound).all()):
        bad.append("the whole product misses its bound")
    img = img0.copy()
    edges = [c for c in cuts if c < m_full] + [m_full]
    plans = _runs.setdefault("rowblock", {})
    for r0, r1 in zip(edges[:-1], edges[1:]):
        before = img.copy()
        img, plan = view(A, B, img, m=r1 - r0, form=3, m_full=m_full, r0=r0, **kw)
        blk = gc.replace(whole, form=3, m=r1 - r0, m_full=m_full, r0=r0, tag="cut%d" % cuts[1])
        print("%s plan=%s" % (blk.id, [plan[f] for f in gc.PLAN_FIELDS]))
        plans[blk.id] = (blk, plan, [], None)
        if plan["wide"] != 1 - (r0 & 1):
            bad.append("rows from %d: wide = %d" % (r0, plan["wide"]))
        a, b = before.copy(), img.copy()            # nothing but rows [r0, r1) of the view changed
        gc.view_of(whole, a)[r0:r1] = 0.0
        gc.view_of(whole, b)[r0:r1] = 0.0
        if not gc._same_bits(a, b):
            bad.append("rows [%d, %d): wrote outside the block" % (r0, r1))
    same = gc._same_bits(gc.view_of(whole, img), ref)
    _rowblock_record["rowblock-%dx%dx%d-cut%d" % (m_full, k, l, cuts[1])] = bool(same)
    if not same:
        bad.append("%d entries differ in bits from the one launch" % int((gc.view_of(whole, img) != ref).sum()))
    _rowblock_runs[(shape, cuts)] = bad
    return bad


@pytest.mark.parametrize("shape", gc.ROWBLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cuts", gc.ROWBLOCK_CUTS, ids=("aligned", "odd"))
def test_row_blocks_are_bit_identical_to_one_launch(gsi, shape, cuts):
    """gemm_f64_nn_rowblock: blocks computed with the full shape's K split, put together, are the one launch's bits."""
    bad = _run_rowblocks(gsi, shape, cuts)
    assert not bad, bad


def test_table_reaches_every_path(gsi):
    """The union of the plans the launcher reported for the table: every path of the dispatch is in it."""
    for g in gc.GROUPS:
        _run_group(gsi, g)
    for shape in gc.ROWBLOCK_SHAPES:
        for cuts in gc.ROWBLOCK_CUTS:
            _run_rowblocks(gsi, shape, cuts)
    runs = [(c, p) for g in _runs.values() for (c, p, _, _) in g.values()]
    plain = [(c, p) for c, p in runs if c.form == 0]
    missing = []
    for xmode in (0, 1):
        for trans in (False, True):
            for nt in range(1, 11):
                if not any(c.trans == trans and p["nt"] == nt and p["xmode"] == xmode for c, p in plain):
                    missing.append("NT %d %s XMODE %d" % (nt, "TN" if trans else "NN", xmode))
    for trans in (False, True):
        if not any(c.trans == trans and p["xmode"] == 2 for c, p in plain):
            missing.append("XMODE 2 %s" % ("TN" if trans else "NN"))
    for wide in (0, 1):
        for trans in (False, True):
            if not any(c.trans == trans and p["wide"] == wide for c, p in plain):
                missing.append("wide %d %s" % (wide, "TN" if trans else "NN"))
    if not any(p["nsplit"] > 1 and p["nsplit"] % 8 == 0 for _, p in runs):
        missing.append("a split count that is a multiple of 8")
    if not any(p["nsplit"] > 1 and p["nsplit"] % 8 != 0 for _, p in runs):
        missing.append("a split count that is no multiple of 8")
    if not any(p["persistent"] == 1 for _, p in runs):
        missing.append("persistent mode")
    for n in (1, 2, 3):
        if not any(p["nchunks"] == n for _, p in runs):
            missing.append("%d column chunks" % n)
    for form in (1, 2, 3):
        if not any(c.form == form and p["nt"] > 0 for c, p in runs):
            missing.append("form %d" % form)
    assert not missing, missing
