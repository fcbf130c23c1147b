"""The interchanges of a panel LU composed into the power step's index lists: a model of `lr_compose_kernel`.

`lowrank_power.hip: lr_compose_kernel` turns the l pivots of P Y = L U into the index lists that the power step's gather and
check read.  `compose` below is that kernel in Python, with its data structures and its order: every
step j looks up the last earlier step that named position j (`pa`) and the last one that named its own pivot row (`pb`), the
chains of `pa` are resolved by pointer jumping (`up`), the lower positions are taken at the last step that named them and
rank-sorted, a scan over [top; sorted lower positions] numbers the moved rows, the lists are padded with S[0] - S[0] rows,
and the check rows are the splitmix64 sample, looked up by binary search.  It is tested against plainly applying the
interchanges to arange(n).
"""
import numpy as np
import pytest

NSAMPLE = 256
M64 = (1 << 64) - 1


def up8(x):
    return (x + 7) & ~7


def layout(n, l):
    nchk = l + min(NSAMPLE, n - l)
    o_chk = up8(2 * l)
    o_sm = o_chk + up8(nchk)
    ldr = up8(o_sm + 2 * l)
    return nchk, o_chk, o_sm, ldr


def sample_row(n, l, c):
    """the check row of index c >= l: splitmix64 of the (c - l + 1)-th state after the seed, reduced to [l, n)"""
    z = (0x9E3779B97F4A7C15 * (c - l + 2)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return l + z % (n - l)


def compose(piv, n):
    """(src, sub, chk, bad, nmv) as the kernel writes them; -7 marks a slot the kernel would leave unwritten"""
    l = len(piv)
    nchk, o_chk, o_sm, ldr = layout(n, l)
    bad = 0
    pv = []
    for j, r in enumerate(piv):
        if r < j or r >= n:
            bad = 1
            r = j if r < j else n - 1
        pv.append(r)
    top = [None] * l
    BIG = 2 ** 31 - 1
    up, pb, last = [0] * l, [-1] * l, [False] * l
    for j in range(l):                                   # thread j: one pass over the pivots
        r, pa, lst = pv[j], -1, pv[j] >= l
        for jp in range(j):
            if pv[jp] == j:
                pa = jp
            if pv[jp] == r:
                pb[j] = jp
        for jp in range(j + 1, l):
            if pv[jp] == r:
                lst = False
        last[j] = lst
        up[j] = pa if pa >= 0 else j
    span = 1
    while span < l:                                      # pointer jumping, every round from the round before
        up = [up[up[j]] for j in range(l)]
        span <<= 1
    lk, lv = [BIG] * l, [0] * l
    for j in range(l):
        r = pv[j]
        top[j] = up[j] if r == j else (up[pb[j]] if pb[j] >= 0 else r)
        if last[j]:
            lk[j] = r
        lv[j] = up[j]
    cnt = sum(1 for j in range(l) if lk[j] != BIG)
    sk, sv = [None] * cnt, [None] * cnt
    for j in range(l):                                   # rank sort (the keys are distinct)
        if lk[j] != BIG:
            rank = sum(1 for i in range(l) if lk[i] < lk[j])
            sk[rank], sv[rank] = lk[j], lv[j]
    src, sub, chk = [-7] * ldr, [-7] * ldr, [-7] * nchk
    k = 0
    for q in range(l + cnt):                             # the scan: candidates in ascending position
        pos, val = (q, top[q]) if q < l else (sk[q - l], sv[q - l])
        if val == pos:
            continue
        src[k], sub[k] = val, pos
        src[o_sm + k], sub[o_sm + k] = pos, -1
        k += 1
    nmv = k
    for i in range(ldr):
        used = i < nmv or o_chk <= i < o_chk + nchk or o_sm <= i < o_sm + nmv
        if not used:
            src[i] = sub[i] = 0
    for c in range(nchk):
        i = c if c < l else sample_row(n, l, c)
        p = i
        if i < l:
            p = top[i]
        else:
            lo, hi = 0, cnt
            while lo < hi:
                mid = (lo + hi) >> 1
                if sk[mid] < i:
                    lo = mid + 1
                else:
                    hi = mid
            if lo < cnt and sk[lo] == i:
                p = sv[lo]
        chk[c] = i
        src[o_chk + c], sub[o_chk + c] = p, -1
    return np.array(src), np.array(sub), np.array(chk), bad, nmv


def plain_perm(piv, n):
    """(P S)[i] = S[perm[i]] by applying the interchanges one by one"""
    perm = np.arange(n)
    for j, r in enumerate(piv):
        perm[[j, r]] = perm[[r, j]]
    return perm


def host_sample(n, l):
    """the check rows as the host loop of the earlier power step drew them (the state advanced once per row)"""
    h, rows = 0x9E3779B97F4A7C15, []
    for _ in range(min(NSAMPLE, n - l)):
        h = (h + 0x9E3779B97F4A7C15) & M64
        z = h
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        rows.append(l + z % (n - l))
    return rows


def check_against_plain(piv, n):
    piv = [int(r) for r in piv]
    l = len(piv)
    nchk, o_chk, o_sm, ldr = layout(n, l)
    src, sub, chk, bad, nmv = compose(piv, n)
    assert bad == 0
    assert (src != -7).all() and (sub != -7).all() and (chk != -7).all()         # every slot written
    perm = plain_perm(piv, n)
    mv = np.nonzero(perm != np.arange(n))[0]                                     # ascending
    assert nmv == len(mv) <= 2 * l
    assert np.array_equal(sub[:nmv], mv) and np.all(np.diff(sub[:nmv]) > 0)
    assert np.array_equal(src[:nmv], perm[mv])
    assert np.array_equal(src[o_sm:o_sm + nmv], mv) and np.all(sub[o_sm:o_sm + nmv] == -1)
    assert np.array_equal(chk[:l], np.arange(l)) and list(chk[l:]) == host_sample(n, l)
    assert np.array_equal(src[o_chk:o_chk + nchk], perm[chk]) and np.all(sub[o_chk:o_chk + nchk] == -1)
    pad = np.ones(ldr, bool)                                                     # everything else is S[0] - S[0]
    pad[:nmv] = False
    pad[o_chk:o_chk + nchk] = False
    pad[o_sm:o_sm + nmv] = False
    assert np.all(src[pad] == 0) and np.all(sub[pad] == 0)
    assert pad[nmv:2 * l].all() and pad[o_sm + nmv:o_sm + 2 * l].all()
    return nmv


def test_no_interchange():
    assert check_against_plain(range(12), 100) == 0


def test_every_pivot_an_interchange():
    l, n = 16, 400
    assert check_against_plain([l + 3 * j for j in range(l)], n) == 2 * l
    assert check_against_plain([l - 1 - j if j < l // 2 else j for j in range(l)], n) == l    # all within the top block


def test_row_moved_three_times():
    # row 50 goes to position 0, comes back out by way of 1 and 2
    piv = [50, 50, 50, 3, 4, 5]
    check_against_plain(piv, 64)
    perm = plain_perm(piv, 64)
    assert perm[0] == 50 and perm[50] == 2


def test_pivot_brings_an_earlier_row_back():
    # step 0 sends row 0 down to position 9, step 1 fetches it from there: position 9 ends with row 1
    piv = [9, 9, 2, 3]
    assert check_against_plain(piv, 30) == 3
    perm = plain_perm(piv, 30)
    assert list(perm[:2]) == [9, 0] and perm[9] == 1
    # the same through three steps, and within the top block alone
    assert check_against_plain([7, 7, 7, 3], 30) == 4
    assert check_against_plain([3, 3, 2, 3], 16) == 3
    # a row that an interchange took never returns to its own position: moved rows = rows of the non-trivial interchanges
    src, sub, chk, bad, nmv = compose([7, 1, 2, 3, 4], 30)
    assert nmv == 2 and list(sub[:2]) == [0, 7] and list(src[:2]) == [7, 0]


def test_no_interchange_mixed_with_last_row():
    n, l = 90, 10
    check_against_plain([j if j % 2 else n - 1 for j in range(l)], n)


def test_n_equals_2l():
    rng = np.random.default_rng(3)
    for l in (1, 2, 7, 64):
        n = 2 * l
        piv = [int(rng.integers(j, n)) for j in range(l)]
        check_against_plain(piv, n)
    l = 64
    assert check_against_plain([2 * l - 1 - j for j in range(l)], 2 * l) == 2 * l


def test_random_pivot_lists():
    rng = np.random.default_rng(11)
    for trial in range(1000):
        l = int(rng.integers(1, 49))
        n = int(rng.integers(2 * l, 2 * l + (4 if trial % 3 == 0 else 400)))
        piv = [j if rng.random() < 0.15 else int(rng.integers(j, n)) for j in range(l)]
        check_against_plain(piv, n)


def test_largest_l():
    rng = np.random.default_rng(5)
    l, n = 384, 1000000
    check_against_plain([int(rng.integers(j, n)) for j in range(l)], n)


@pytest.mark.parametrize("piv,n", [([3, 0, 2], 10), ([10, 1, 2], 10), ([-1, 5, 2 ** 31 - 1], 10), ([0, 1, 1], 6)])
def test_invalid_pivots_raise_the_flag_and_stay_in_range(piv, n):
    l = len(piv)
    nchk, o_chk, o_sm, ldr = layout(n, l)
    src, sub, chk, bad, nmv = compose(piv, n)
    assert bad == 1
    assert (src >= 0).all() and (src < n).all()
    assert (sub >= -1).all() and (sub < n).all()
    assert (chk >= 0).all() and (chk < n).all()
    assert 0 <= nmv <= 2 * l
    clamped = [min(max(r, j), n - 1) for j, r in enumerate(piv)]
    s2, b2, c2, bad2, nmv2 = compose(clamped, n)
    assert bad2 == 0 and nmv2 == nmv and np.array_equal(s2, src) and np.array_equal(b2, sub) and np.array_equal(c2, chk)
