"""The case table of tests/test_gemm_kernels_gpu.py: gemm_f64_kernel<NT, TRANS_A, 0, XMODE> and its launcher
(csrc/gemm_f64.hip) run through gsi_gemm_view on strided device views, against exact host references.

EXACT cases: A and B hold integers in [-4, 4], C0 integers in [-8, 8], drawn with P(v) rising linearly in v (no symmetry
for a transposed or mirrored fragment to hide behind); alpha in {1, -1, 0.5}, beta in {0, 1, -2}.  Every partial sum is an
integer of at most 16 K <= 2^17, alpha times it a half-integer, so the product is exact in fp64 in ANY summation order, K
splits and FMA included; the reference is an int64 matmul.  REAL cases: standard-normal A, B, C0 against np.longdouble
(64-bit mantissa: its own error <= K 2^-64 per unit of |A||B|, under 1/2000 of the bound) with the entrywise bound
    |C - ref| <= gamma_(K+2) (|alpha| |A||B| + |beta| |C0|),   gamma_n = n u / (1 - n u),  u = 2^-53:
the textbook bound of an inner product of length K in any order (Higham, Accuracy and Stability, section 3.1; an FMA only
removes roundings) plus the two roundings of the alpha / beta update.

A case describes the DEVICE layout: leading dimensions and element offsets into 16-byte-aligned allocations whose
padding is NaN (operands) or a recognisable image (C).  `expect` lists plan fields the launcher must report for it;
test_table_reaches_every_path takes the union of the reported plans.  run_case / check_case need only something with
gemm_view's signature, so tests/test_gemm_cases.py runs every check on the CPU against a numpy stand-in."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, replace

import numpy as np

U = 2.0 ** -53
ALPHAS = (1.0, -1.0, 0.5)
BETAS = (0.0, 1.0, -2.0)
AB = tuple((a, b) for a in ALPHAS for b in BETAS)
M_AXIS = (1, 127, 128, 129, 257)
K_AXIS = (1, 31, 32, 33, 64, 65, 96, 97, 129, 161)
PLAN_FIELDS = ("nt", "nchunks", "xmode", "wide", "nsplit", "persistent", "grid_x", "active")


@dataclass(frozen=True)
class Case:
    group: str
    m: int                      # rows of C (form 3: rows of the block)
    l: int                      # columns of C
    k: int                      # reduction length
    form: int = 0               # 0 gemm, 1 syrk upper (C = A'A, m == l), 2 trmm upper, 3 NN row block
    trans: bool = False
    alpha: float = 1.0
    beta: float = 0.0
    lda: int = 0                # 0: packed (the rows of the stored operand)
    ldb: int = 0
    ldc: int = 0
    a_off: int = 0
    b_off: int = 0
    c_off: int = 0
    real: bool = False
    seed: int = 0
    lpool: int = 0              # B is the first l of lpool drawn columns (cases that share one reference product)
    krep: int = 1               # A = [A0 A0 ... A0], krep copies along the reduction (large K without a large draw)
    upper: bool = False         # B upper triangular, zeros below the diagonal (always so for form 2)
    m_full: int = 0             # form 3
    r0: int = 0
    expect: tuple = ()          # ((plan field, value), ...)
    tag: str = ""

    @property
    def tn(self):               # the stored operand is (reduction x rows)
        return self.trans or self.form == 1

    @property
    def a_rows(self):
        return self.m_full if self.form == 3 else (self.k if self.tn else self.m)

    @property
    def a_cols(self):
        return self.m if self.tn else self.k

    @property
    def c_rows(self):
        return self.m_full if self.form == 3 else self.m

    @property
    def LDA(self):
        return self.lda or self.a_rows

    @property
    def LDB(self):
        return self.ldb or self.k

    @property
    def LDC(self):
        return self.ldc or self.c_rows

    @property
    def image_doubles(self):
        return self.c_off + self.LDC * self.l

    @property
    def id(self):
        s = "%s-f%d-%s-m%d-l%d-k%d" % (self.group, self.form, "tn" if self.trans else "nn", self.m, self.l, self.k)
        s += "-a%g-b%g" % (self.alpha, self.beta)
        s += "-ld%d.%d.%d-off%d.%d.%d" % (self.LDA, self.LDB, self.LDC, self.a_off, self.b_off, self.c_off)
        if self.form == 3:
            s += "-of%d-r%d" % (self.m_full, self.r0)
        return s + ("-real" if self.real else "") + (("-" + self.tag) if self.tag else "")


def ld(rows, odd):
    """rows + 3 or rows + 4, whichever has the wanted parity."""
    return rows + 3 if (rows + 3) % 2 == int(bool(odd)) else rows + 4


def _layout(m, l, k, trans, a=(0, 0), b=(0, 0), c=(0, 0)):
    """(odd offset?, odd leading dimension?) per operand -> the keyword arguments of a Case."""
    ar = k if trans else m
    return dict(lda=ld(ar, a[1]), ldb=ld(k, b[1]), ldc=ld(m, c[1]), a_off=2 + a[0], b_off=2 + b[0], c_off=2 + c[0])


# ------------------------------------------------------------------------------------------------ the table
def _nt_group():
    """NT 1..10 in one chunk: full, one column short, one column into the last tile; aligned and unaligned operators."""
    out, i = [], 0
    for nt in range(1, 11):
        for trans in (False, True):
            for l in (16 * nt, 16 * nt - 1, 16 * (nt - 1) + 1):
                m, k = M_AXIS[i % 5], K_AXIS[(3 * i + i // 10) % 10]
                al, be = AB[i % 9]
                full = l == 16 * nt
                base = dict(group="nt", m=m, l=l, k=k, trans=trans, alpha=al, beta=be, seed=i)
                out.append(Case(**base, **_layout(m, l, k, trans),
                                expect=(("nt", nt), ("nchunks", 1), ("xmode", 0 if full else 1), ("wide", 1))))
                # the operator only 8-byte aligned: by its leading dimension, or by its base
                how = ((0, 1), (1, 0))[(i + nt) % 2] if not full else ((0, 1), (1, 0), (1, 1))[i % 3]
                out.append(Case(**base, **_layout(m, l, k, trans, a=how),
                                expect=(("nt", nt), ("nchunks", 1), ("xmode", 0), ("wide", 0))))
                i += 1
    out.append(replace(out[7], real=True, beta=-2.0))
    out.append(replace(out[-20], real=True, alpha=0.5))
    return out


def _rows_group():
    """Every row count against every reduction depth (1 to 6 reduction tiles, even and odd), NN and TN."""
    out, i = [], 0
    for m in M_AXIS:
        for k in K_AXIS:
            al, be = AB[i % 9]
            l = (48, 37)[i % 2]
            c = ((0, 0), (1, 1), (0, 1), (1, 0))[i % 4]
            out.append(Case(group="rows", m=m, l=l, k=k, alpha=al, beta=be, seed=100 + i,
                            **_layout(m, l, k, False, a=(0, (i // 2) % 2), c=c)))
            for odd in (0, 1):          # TN: 16-byte loads with a partial last tile (K odd, lda even), and element-wise
                out.append(Case(group="rows", m=m, l=l, k=k, trans=True, alpha=al, beta=be, seed=100 + i,
                                **_layout(m, l, k, True, a=(0, odd), c=c), expect=(("wide", 1 - odd),)))
            i += 1
    out.append(replace(out[3 * 29], real=True))
    out.append(replace(out[3 * 47 + 1], real=True))
    return out


def _align_group():
    """Base offset and leading-dimension parity of each operand, alone and in every combination."""
    out, i = [], 0
    m, k = 129, 65
    for bits in range(64):
        f = [(bits >> j) & 1 for j in range(6)]
        a, b, c = (f[0], f[1]), (f[2], f[3]), (f[4], f[5])
        for trans in (False, True):
            l = (48, 47)[i % 2]
            a_ok, b_ok = not any(a), not any(b)
            xmode = (0 if (b_ok and l % 48 == 0) else 1) if a_ok else 0
            al, be = AB[i % 9]
            out.append(Case(group="align", m=m, l=l, k=k, trans=trans, alpha=al, beta=be, seed=300 + i,
                            **_layout(m, l, k, trans, a=a, b=b, c=c),
                            expect=(("nt", 3), ("xmode", xmode), ("wide", int(a_ok)))))
            i += 1
    out.append(replace(out[2 * 0b101101], real=True, beta=1.0))
    return out


def _chunks_group():
    out, i = [], 0
    for (m, l, k, exp) in ((257, 161, 97, (("nt", 6), ("nchunks", 2), ("xmode", 1))),
                           (257, 192, 97, (("nt", 6), ("nchunks", 2), ("xmode", 0))),
                           (257, 320, 97, (("nt", 10), ("nchunks", 2), ("xmode", 0))),
                           (257, 400, 97, (("nt", 9), ("nchunks", 3), ("xmode", 1))),
                           (257, 480, 97, (("nt", 10), ("nchunks", 3), ("xmode", 0))),
                           (1100, 320, 64, (("nt", 10), ("nchunks", 2), ("active", 18)))):
        for trans in (False, True):
            al, be = AB[(2 * i + 1) % 9]
            out.append(Case(group="chunks", m=m, l=l, k=k, trans=trans, alpha=al, beta=be, seed=500 + i,
                            **_layout(m, l, k, trans), expect=exp + (("nsplit", 1), ("persistent", 0))))
            i += 1
    out.append(replace(out[6], real=True))
    return out


def _split_group():
    out, i = [], 0
    for (m, l, k, ns) in ((100, 48, 256, 2), (100, 48, 400, 3), (100, 48, 1024, 8), (100, 48, 1030, 7), (300, 160, 2048, 16),
                          (129, 320, 700, 5)):
        for trans in (False, True):
            al, be = AB[(4 * i + 2) % 9]
            out.append(Case(group="split", m=m, l=l, k=k, trans=trans, alpha=al, beta=be, seed=600 + i,
                            **_layout(m, l, k, trans), expect=(("nsplit", ns),)))
            i += 1
    # the update of the sample-space power step: TN, beta = 1, views of wider matrices
    out.append(Case(group="split", m=1024, l=320, k=640, trans=True, beta=1.0, lda=2500, ldc=2500, ldb=ld(640, 0), seed=620,
                    expect=(("nsplit", 5), ("nchunks", 2))))
    # the trailing update of the panel factorizations: alpha = -1, beta = 1
    for trans in (False, True):
        out.append(Case(group="split", m=100, l=48, k=1024, trans=trans, alpha=-1.0, beta=1.0, seed=621,
                        **_layout(100, 48, 1024, trans, c=(1, 1)), expect=(("nsplit", 8),)))
    out.append(replace(out[4], real=True, alpha=-1.0, beta=1.0))
    out.append(replace(out[7], real=True, alpha=0.5, beta=-2.0))
    return out


def _persistent_group():
    """512 output tiles and more on one K split: the work-item loop of the persistent mode."""
    out = []
    for nt in range(1, 11):
        for trans in (False, True):
            al, be = AB[(nt + 4 * trans) % 9]
            odd = int((nt, trans) in ((3, False), (7, True)))       # two of them element-wise
            out.append(Case(group="persistent", m=65537, l=16 * nt, k=33, trans=trans, alpha=al, beta=be, seed=700, lpool=160,
                            lda=ld(33 if trans else 65537, odd), ldb=ld(33, 0), ldc=ld(65537, nt % 2),
                            expect=(("nt", nt), ("xmode", 0), ("wide", 1 - odd), ("persistent", 1), ("nsplit", 1),
                                    ("active", 513))))
    for trans in (False, True):
        out.append(Case(group="persistent", m=32891, l=320, k=96, trans=trans, alpha=-1.0, beta=1.0, seed=701,
                        lda=ld(96 if trans else 32891, 0), ldb=ld(96, 0), ldc=ld(32891, 0),
                        expect=(("nt", 10), ("nchunks", 2), ("persistent", 1), ("active", 514))))
    out.append(replace(out[0], real=True))
    return out


def _deep_group():
    """The persistent group's row counts with a reduction of more than 128 tiles: the launcher leaves the mode."""
    out = []
    for trans in (False, True):
        out.append(Case(group="deep", m=65537, l=16, k=4128, krep=32, trans=trans, seed=702,
                        lda=ld(4128 if trans else 65537, 0), ldb=ld(4128, 0), ldc=ld(65537, 0),
                        expect=(("nt", 1), ("persistent", 0))))
    # ... also where the chooser leaves K whole (512 output tiles: two full rounds), so that the depth alone decides
    out.append(Case(group="deep", m=65536, l=16, k=4128, krep=32, seed=703, lda=ld(65536, 0), ldb=ld(4128, 0),
                    ldc=ld(65536, 0), expect=(("nt", 1), ("persistent", 0), ("nsplit", 1), ("xmode", 0), ("active", 512))))
    out.append(Case(group="deep", m=300, l=16, k=4128, real=True, seed=704, **_layout(300, 16, 4128, False)))
    return out


def _tri1_group():
    out = []
    for i, ((l, mred, ns), odd) in enumerate(zip(((96, 300, 2), (128, 4096, 26), (320, 5000, 32), (384, 5000, 32), (95, 70, 1)),
                                                 (0, 1, 0, 1, 1))):
        out.append(Case(group="tri1", form=1, m=l, l=l, k=mred, lda=ld(mred, odd), ldc=ld(l, i % 2), a_off=2 + (i == 3),
                        c_off=2 + (i % 3 == 0), seed=800 + i, expect=(("nsplit", ns),)))
    out.append(replace(out[0], real=True))
    return out


def _tri2_group():
    """B upper triangular: form 2 and, on the same operands, form 0 (the two must agree bit for bit)."""
    out, i = [], 0
    for kl in (33, 160, 161, 320, 400):
        for m in (129, 1100):
            for form in (2, 0):
                out.append(Case(group="tri2", form=form, upper=True, m=m, l=kl, k=kl, seed=900 + i,
                                **_layout(m, kl, kl, False, a=(0, i % 2), b=(0, (i // 2) % 2), c=(i % 2, 0))))
            i += 1
    out.append(replace(out[4], real=True))
    out.append(replace(out[5], real=True))
    return out


LD_EDGES = (("ldb", False, 3355442, 3355443), ("lda", True, 4194302, 4194303), ("lda", False, 16777211, 16777212))


def _bigld_group():
    """The last leading dimension the 32-bit tile offsets reach and the first that needs XMODE 2:
    8 (160 ldb + 32) >= 2^32, 8 ((TN ? 128 : 32) lda + 128) >= 2^32.  L = 160: all ten column tiles, the largest offsets."""
    out = []
    for i, (which, trans, last32, first64) in enumerate(LD_EDGES):
        for ldv, xmode in ((last32, 0), (first64, 2)):
            m, k = (100, 64) if which == "ldb" else ((128, 64) if trans else (128, 8))
            al, be = AB[(i + 5 * (xmode == 2)) % 9]
            kw = dict(lda=ld(k if trans else m, 0), ldb=ld(k, 0))
            kw[which] = ldv
            out.append(Case(group="bigld", m=m, l=160, k=k, trans=trans, alpha=al, beta=be, seed=1000 + i, **kw,
                            expect=(("nt", 10), ("xmode", xmode), ("wide", 1 - (kw["lda"] & 1)))))
    out.append(replace(out[1], real=True))
    return out


GROUPS = {"nt": _nt_group, "rows": _rows_group, "align": _align_group, "chunks": _chunks_group, "split": _split_group,
          "persistent": _persistent_group, "deep": _deep_group,
          "tri1": _tri1_group, "tri2": _tri2_group, "bigld": _bigld_group}
BIG_GROUPS = ("persistent", "deep", "bigld")            # the only ones whose device footprint is more than a few MB
# row blocks (form 3): (M_full, K, L), both products split; cuts at multiples of 128 and at odd rows
ROWBLOCK_SHAPES = ((1000, 700, 48), (300, 2048, 160))
ROWBLOCK_CUTS = ((0, 128, 256, 384, 512, 640, 768, 896), (0, 77, 333, 590, 847))


@functools.lru_cache(maxsize=None)
def group_cases(group):
    cases = tuple(GROUPS[group]())
    assert len({c.id for c in cases}) == len(cases), "duplicate case ids in " + group
    return cases


def all_cases():
    return tuple(c for g in GROUPS for c in group_cases(g))


# ------------------------------------------------------------------------------------------------ operands
def _draw_ints(rng, shape, half):
    vals = np.arange(-half, half + 1)
    p = np.arange(1.0, vals.size + 1.0)
    return rng.choice(vals, size=shape, p=p / p.sum()).astype(np.int64)


def _threaded_rows(fn, rows):
    """fn(r0, r1) over row ranges on a few threads (numpy's integer and long-double matmuls are plain loops that release the GIL)."""
    nthreads = max(1, min(16, os.cpu_count() or 1))
    if rows < 64:
        return [fn(0, rows)]
    cuts = np.linspace(0, rows, 4 * nthreads + 1).astype(int)
    with ThreadPoolExecutor(nthreads) as ex:
        return list(ex.map(lambda i: fn(cuts[i], cuts[i + 1]), range(cuts.size - 1)))


def matmul_rows(A, B):
    """A @ B in the dtype of the operands (int64 or long double), row ranges in parallel."""
    A = np.ascontiguousarray(A)
    B = np.asfortranarray(B)
    return np.concatenate(_threaded_rows(lambda r0, r1: A[r0:r1] @ B, A.shape[0]), axis=0)


@functools.lru_cache(maxsize=3)
def _pool(seed, m, k0, kpool, lpool, real, c_doubles):
    """Logical op(A)'s first k0 reduction indices (m x k0), B (kpool x lpool), and the C image, by seed and shape alone."""
    rng = np.random.default_rng(seed)
    if real:
        return rng.standard_normal((m, k0)), rng.standard_normal((kpool, lpool)), rng.standard_normal(c_doubles)
    return _draw_ints(rng, (m, k0), 4), _draw_ints(rng, (kpool, lpool), 4), _draw_ints(rng, c_doubles, 8).astype(np.float64)


@functools.lru_cache(maxsize=3)
def _int_product(seed, m, k0, kpool, lpool, krep, c_doubles, form, upper):
    A0, B, _ = _pool(seed, m, k0, kpool, lpool, False, c_doubles)
    if form == 1:
        return matmul_rows(B.T, B)
    if upper:
        B = np.triu(B)
    Bs = B.reshape(krep, k0, lpool).sum(axis=0)             # A = [A0 ... A0]: A B = A0 (sum of B's row blocks)
    return matmul_rows(A0, Bs)


def _pool_key(case):
    assert case.k % case.krep == 0
    rows = case.m_full if case.form == 3 else case.m
    return (case.seed, rows, case.k // case.krep, case.k, case.lpool or case.l, case.real)


def operands(case):
    """(A as stored: packed, column-major; B packed or None; the C image before the launch; C0 = its m x l view, NaN-free)."""
    A0, B, img = _pool(*_pool_key(case), case.image_doubles)
    B = B[:, :case.l]
    if case.form == 1:                                      # the one stored operand is the k x l matrix itself
        A_st, B_st = np.asfortranarray(B, dtype=np.float64), None
    else:
        assert case.upper or case.form != 2
        if case.upper:
            B = np.triu(B)
        # op(A) = [A0 ... A0] (m x k).  TN stores its transpose: the row-major tiling read column-major
        if case.tn:
            A_st = np.tile(A0.astype(np.float64), (1, case.krep)).T
        else:
            A_st = np.tile(np.ascontiguousarray(A0.T, dtype=np.float64), (case.krep, 1)).T
        B_st = np.asfortranarray(B, dtype=np.float64)
    img = np.array(img, dtype=np.float64)
    C0 = view_of(case, img).copy()
    if case.beta == 0.0:
        img[:] = np.nan                                     # beta == 0 must not read C: whatever it read would show
    return A_st, B_st, img, C0


def view_of(case, img, rows=None):
    """The c_rows x l view of C inside its image."""
    return img[case.c_off:case.c_off + case.LDC * case.l].reshape((case.LDC, case.l), order="F")[:rows or case.c_rows]


def run_case(gemm_view, case):
    """-> (image before, image after, plan, operands)."""
    A_st, B_st, img0, C0 = operands(case)
    img, plan = gemm_view(A_st, B_st, img0, m=case.m, l=case.l, k=case.k, form=case.form, trans=case.trans, alpha=case.alpha,
                          beta=case.beta, lda=case.LDA, a_off=case.a_off, ldb=case.LDB, b_off=case.b_off, ldc=case.LDC,
                          c_off=case.c_off, m_full=case.m_full, r0=case.r0)
    return img0, img, plan, (A_st, B_st, C0)


# ------------------------------------------------------------------------------------------------ checks
def _same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64))


def outside_untouched(case, img0, img):
    """Every double of the image outside the m x l view holds the bits that were uploaded."""
    a, b = img0.copy(), img.copy()
    view_of(case, a)[:] = 0.0
    view_of(case, b)[:] = 0.0
    return _same_bits(a, b)


def gamma(n):
    return n * U / (1.0 - n * U)


def check_case(case, img0, img, plan, ops):
    """-> (list of failures, error / bound ratio of a real case or None)."""
    A_st, B_st, C0 = ops
    bad = []
    for field, want in case.expect:
        if plan is not None and plan[field] != want:
            bad.append("plan.%s = %d, expected %d" % (field, plan[field], want))
    if plan is not None and case.form == 0 and "persistent" in dict(case.expect) and plan["persistent"]:
        if not plan["grid_x"] < plan["active"]:
            bad.append("persistent with grid.x %d for %d output tiles" % (plan["grid_x"], plan["active"]))
    if not outside_untouched(case, img0, img):
        bad.append("memory outside the view of C was written")
    got = view_of(case, img)
    keep = np.triu(np.ones((case.l, case.l), dtype=bool)) if case.form == 1 else np.ones(got.shape, dtype=bool)
    if not np.isfinite(got[keep]).all():
        bad.append("non-finite entries in the result (%d)" % int((~np.isfinite(got[keep])).sum()))
        return bad, None
    ratio = None
    if not case.real:
        P = _int_product(*_pool_key(case)[:5], case.krep, case.image_doubles, case.form, case.upper)[:, :case.l]
        ref = case.alpha * P.astype(np.float64)
        if case.beta != 0.0:
            ref = ref + case.beta * C0
        if not np.array_equal(got[keep], ref[keep]):
            w = np.argwhere((got != ref) & keep)
            bad.append("%d entries differ from the int64 product, first at %s: %r != %r"
                       % (len(w), tuple(w[0]), got[tuple(w[0])], ref[tuple(w[0])]))
    else:
        ld_ = np.longdouble
        if case.form == 1:
            opA, Bm = A_st.T, A_st
        else:
            opA, Bm = (A_st.T if case.tn else A_st), B_st
        ref = case.alpha * matmul_rows(opA.astype(ld_), Bm.astype(ld_))
        mag = abs(case.alpha) * matmul_rows(np.abs(opA).astype(ld_), np.abs(Bm).astype(ld_))
        if case.beta != 0.0:
            ref = ref + case.beta * C0.astype(ld_)
            mag = mag + abs(case.beta) * np.abs(C0).astype(ld_)
        bound = gamma(case.k + 2) * mag
        err = np.abs(got.astype(ld_) - ref)
        ratio = float((err[keep] / bound[keep]).max())
        if not (err[keep] <= bound[keep]).all():
            bad.append("%d entries beyond gamma_(K+2) (|alpha||A||B| + |beta||C0|), largest ratio %.3g"
                       % (int((err > bound)[keep].sum()), ratio))
    return bad, ratio
