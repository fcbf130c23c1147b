"""tests/pointcov_model.py on the CPU: the tiling model against the figures the sources state, the reach of the case table
of test_pointcov_kernels_gpu.py (GEN 2 and all eight pointcov_wide_kernel<NTQ, MT, RGN> instantiations, each with one split
and with several; every short-reduction class for both prefetch schedules; ragged and full edges; offsets under the
diagonal test; a rank without rows), the conditions the point sets must meet, the reference against mpmath, and the
harness itself on the CPU reference backend (the same two assertions the GPU test makes)."""
import numpy as np
import pytest

import cpuref
import pointcov_model as pm

WIDE = [(4, 3, 4), (5, 3, 4), (3, 3, 2), (4, 3, 2), (5, 3, 2), (3, 2, 2), (4, 2, 2), (5, 2, 2)]


def all_launches():
    return [(c, which, rank, m) for c in pm.CASES for which, rank, m in pm.launches(c)]


def wide_launches():
    return [(c, which, rank, m) for c, which, rank, m in all_launches() if m is not None and m["kernel"] != pm.GEN2]


def tile_class(t):
    return {1: "1", 2: "2", 3: "3"}.get(t, "even>=4" if t % 2 == 0 else "odd>=5")


def test_tiling_model_against_the_sources():
    # NTQ and column chunks as the issue and wide_tiling's comments give them
    got = [(pm.wide_tiling(500, l, 500)["ntq"], pm.wide_tiling(500, l, 500)["nchunks"]) for l in (161, 192, 200, 256, 257, 320, 321, 400, 641)]
    assert got == [(3, 1), (3, 1), (4, 1), (4, 1), (5, 1), (5, 1), (3, 2), (4, 2), (4, 3)]
    assert [pm.wide_tiling(500, l, 500)["ntq"] for l in (97, 128, 129, 160)] == [4, 4, 5, 5]
    assert not pm.wide_applies(96) and pm.wide_applies(97) and not pm.wide_applies(320, wide_on=False)
    # the benchmark's product: 2110 row blocks of 96 rows at n = 202 500 (wide_tiling's comment), and it is split
    w = pm.wide_tiling(202500, 320, 202500)
    assert w["active"] == 2110 and w["nsplit"] >= 2 and w["kchunk"] % 32 == 0
    # below K / sp >= 4096 the chooser never splits; at n = 8192 it does
    assert pm.wide_tiling(5000, 320, 5000)["ns_eff"] == 1
    m = pm.launches(pm.NATURAL)[0][2]
    assert m["kernel"] == (5, 3, 2) and m["ns_eff"] >= 2
    # the columns of the one one-hot product straddle the boundary of the first two splits
    cols = pm.onehot_columns(pm.NATURAL, pm.onehot_bases(pm.NATURAL)[0])
    assert cols.min() < m["kchunk"] <= cols.max()
    # forced splits: kchunk is a multiple of 32, so a short reduction takes fewer splits than asked for
    m = pm.model(40, 200, 40, forced=3)
    assert (m["ns_eff"], m["ntiles"], m["last_split"]) == (2, (1, 2), (1, True))


def test_table_reaches_every_kernel_with_one_split_and_with_several():
    kernels = {m["kernel"] for _, _, _, m in all_launches() if m is not None}
    assert kernels == set(WIDE) | {pm.GEN2}
    for inst in WIDE:
        ns = {m["ns_eff"] > 1 for _, _, _, m in wide_launches() if m["kernel"] == inst}
        assert ns == {False, True}, inst
    assert any(m["ns_eff"] >= 3 for _, _, _, m in wide_launches())
    # GEN 2 also at l = 200 and 320 (GSI_POINTCOV_WIDE=0)
    assert {c.l for c, _, _, m in all_launches() if m is not None and m["kernel"] == pm.GEN2} >= {16, 96, 200, 320}


def test_table_reaches_every_short_reduction_for_both_schedules():
    for ns in (1, 2):
        classes = {tile_class(t) for _, _, _, m in wide_launches() if m["NS"] == ns for t in m["ntiles"]}
        assert classes == {"1", "2", "3", "even>=4", "odd>=5"}, (ns, classes)
    # and the 64-row kernels each see one, two and three tiles
    for inst in WIDE[5:]:
        assert {t for _, _, _, m in wide_launches() if m["kernel"] == inst for t in m["ntiles"]} >= {1, 2, 3}, inst


def test_table_reaches_the_edges():
    wl = wide_launches()
    for mt_rgn in {(i[1], i[2]) for i in WIDE}:
        sub = [(c, m) for c, _, _, m in wl if m["kernel"][1:] == mt_rgn]
        assert {m["ragged_rows"] for _, m in sub} == {False, True}, mt_rgn
        assert {m["ragged_cols"] for _, m in sub} == {False, True}, mt_rgn
        assert {m["unused_cols"] > 0 for _, m in sub} == {False, True}, mt_rgn
        assert any(m["M"] > m["BM"] for _, m in sub), mt_rgn                       # more than one row block
        # every kind and every dimension with every arrangement
        assert {c.kind for c, _ in sub} == set(pm.KINDS) and {c.d for c, _ in sub} == {1, 2, 3}, mt_rgn
        assert {c.offset for c, _ in sub} == {False, True}
    assert {m["nchunks"] for _, _, _, m in wl} == {1, 2, 3}
    for mt in (2, 3):
        assert {m["nchunks"] for _, _, _, m in wl if m["kernel"][1] == mt and m["kernel"][2] == 2} >= {1, 2}
    # forced splits whose last split is one ragged tile, and whose last split has several tiles
    forced = [m for c, _, _, m in wl if pm.ENVS[c.env].forced]
    assert any(m["ns_eff"] > 1 and m["last_split"] == (1, True) for m in forced)
    assert any(m["ns_eff"] > 1 and m["last_split"][0] >= 3 for m in forced)
    assert {c.n for c in pm.CASES if pm.ENVS[c.env].forced and pm.ENVS[c.env].ranks == 1} == {40, 100, 200}


def test_table_reaches_offsets_under_the_diagonal_test_and_a_rank_without_rows():
    wl = wide_launches()
    for mt_rgn in {(i[1], i[2]) for i in WIDE}:
        sub = [m for _, _, _, m in wl if m["kernel"][1:] == mt_rgn]
        assert any(m["diag"] and m["roff"] != 0 for m in sub), mt_rgn
        assert any(m["diag"] and m["koff"] != 0 for m in sub), mt_rgn
        assert any(m["diag"] and m["roff"] != 0 and m["ns_eff"] > 1 for m in sub), mt_rgn
        assert any(m["diag"] and m["koff"] != 0 and m["ns_eff"] > 1 for m in sub), mt_rgn
    assert any(which == "none" for _, which, _, _ in all_launches())
    assert pm.shard(2, 3, 2) == (2, 0) and [pm.shard(100, 3, r)[1] for r in range(3)] == [34, 34, 32]
    # K = 32 in the transposed product of n = 100
    assert any(m["K"] == 32 and which == "mul_t" for c, which, _, m in wl if c.n == 100)
    ranks3 = {(c.n, c.l) for c in pm.CASES if pm.ENVS[c.env].ranks == 3}
    assert {n for n, _ in ranks3} == {2, 100, 200, 333} and {l for _, l in ranks3} == {128, 200, 320}


def test_every_group_is_small():
    assert set(pm.GROUPS) == {c.group for c in pm.CASES}
    assert len({pm.case_id(c) for c in pm.CASES}) == len(pm.CASES)
    for c in pm.CASES:
        assert c.n <= 400 or c is pm.NATURAL
        assert len(pm.onehot_bases(c)) <= 9
        if c.n <= 2048:                                   # the one-hot products select every reduction index
            sel = np.concatenate([pm.onehot_columns(c, b) for b in pm.onehot_bases(c)])
            assert set(sel.tolist()) == set(range(c.n)), c


def test_reference_against_mpmath():
    import mpmath
    pm.check_longdouble()
    mpmath.mp.prec = 120
    for case in (pm.CASES[7], pm.CASES[8], pm.CASES[21], pm.CASES[22], pm.CASES[30], pm.CASES[35]):
        P = pm.points(case)
        A, arg, _ = pm.case_reference(case)
        rng = np.random.default_rng(3)
        pairs = [(0, 0)] + [tuple(rng.integers(0, case.n, size=2)) for _ in range(12)]
        for i, j in pairs:
            d2 = sum((mpmath.mpf(float(P[a, i])) - mpmath.mpf(float(P[a, j]))) ** 2 for a in range(case.d))
            r = mpmath.sqrt(d2) / mpmath.mpf(pm.ELL)
            if case.kind == "gaussian":
                a, poly = r * r / 2, 1
            else:
                a = r * mpmath.sqrt({"exponential": 1, "matern32": 3, "matern52": 5}[case.kind])
                poly = {"exponential": 1, "matern32": 1 + a, "matern52": 1 + a + a * a / 3}[case.kind]
            v = mpmath.mpf(pm.SIGMA2) * poly * mpmath.exp(-a) + (mpmath.mpf(pm.NUGGET) if i == j else 0)
            assert abs(mpmath.mpf(float(arg[i, j])) - a) <= 1e-15 * max(a, 1)
            if v > mpmath.mpf(2) ** -900:
                hi = float(A[i, j])
                got = mpmath.mpf(hi) + mpmath.mpf(float(A[i, j] - pm.LD(hi)))
                # long double: exp's argument carries 2^-64 relative, so the value carries ~arg 2^-64
                assert abs(got - v) <= v * (4 + float(a)) * mpmath.mpf(2) ** -62, (case, i, j)


def _distinct_point_sets():
    seen, out = set(), []
    for c in pm.CASES:
        key = (c.kind, c.d, c.n, c.offset)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_point_sets_meet_their_conditions_and_fp64_meets_the_bar():
    """From the reference alone: at most 10 % of a case's entries leave the relative check, the far tail and exact
    underflow are present where the set has far points, coincident pairs exist off the diagonal; and the plain fp64 formula
    (pointcov::kernel's association) stays inside the entry bar and the tail rule, so the reference does."""
    worst = 0.0
    for c in _distinct_point_sets():
        P = pm.points(c)
        cols = pm.onehot_columns(c, pm.onehot_bases(c)[0]) if c.n > 2048 else None
        A, arg, bar = pm.case_reference(c, cols)
        rel = pm.relative_mask(A)
        assert 1.0 - rel.mean() <= pm.MAX_TAIL_FRACTION, (c, 1.0 - rel.mean())
        if c.n >= 64:
            assert (arg > 760).any() and ((arg > 100) & rel).any(), c
            if cols is None:                                         # eight coincident pairs, both orders
                assert ((arg == 0) & ~np.eye(c.n, dtype=bool)).sum() >= 16, c
        F = pm.fp64_formula(P, c.kind, cols)
        worst = max(worst, pm.check_entries(F, A, arg, bar))
    print("fp64 formula: largest ratio to the entry bar %.3f (in units of 2^-53 (1 + arg + delta): %.2f)" % (worst, 16 * worst))
    assert worst <= 1.0


def test_checks_catch_a_misplaced_nugget_a_swapped_pair_and_a_relative_error():
    c = next(c for c in pm.CASES if c.n == 400)
    A, arg, bar = pm.case_reference(c)
    G = np.array(A, dtype=np.float64)
    assert pm.check_entries(G, A, arg, bar) <= 1.0
    i, j = [(i, j) for i, j in zip(*np.nonzero(arg == 0)) if i != j][0]
    B = G.copy(); B[i, j] += pm.NUGGET                        # nugget on a coincident off-diagonal pair
    with pytest.raises(AssertionError):
        pm.check_entries(B, A, arg, bar)
    small = np.unravel_index(int(np.argmin(np.where(pm.relative_mask(A), A, np.inf))), A.shape)
    B = G.copy(); B[small] *= 1.0 + 1e-9                       # 1e-9 relative in the smallest entry of the relative check
    with pytest.raises(AssertionError):
        pm.check_entries(B, A, arg, bar)
    B = G.copy(); B[[0, 1]] = B[[1, 0]]                        # two rows (lanes) swapped
    with pytest.raises(AssertionError):
        pm.check_entries(B, A, arg, bar)
    B = G.copy(); B[arg > 760] = 5e-324                       # not exactly zero beyond the underflow
    with pytest.raises(AssertionError):
        pm.check_entries(B, A, arg, bar)
    X = pm.normal_panel(c)
    Y = np.array(A @ X.astype(pm.LD), dtype=np.float64)
    assert pm.check_product(Y, X, A, bar) <= 1.0
    Y[3, 2] += 1e-9 * abs(Y[3, 2]) + 1e-12
    with pytest.raises(AssertionError):
        pm.check_product(Y, X, A, bar)


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    assert lib.gsi_backend_name().startswith(b"cpu-reference")
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()


def _single_rank_shapes():
    """The single-rank cases as the CPU backend sees them: it has no knobs, so cases that differ only in their environment
    are one."""
    seen, out = set(), []
    for c in pm.CASES:
        key = (c.kind, c.d, c.n, c.l, c.offset)
        if pm.ENVS[c.env].ranks == 1 and c is not pm.NATURAL and key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _single_rank_shapes(), ids=pm.case_id)
def test_harness_on_the_cpu_reference_backend(gsi, cx, case):
    rec = pm.check_case(case, pm.run_case(gsi, cx, case))
    assert rec["bit_identical"]                           # one code path for A X and A' X on this backend
