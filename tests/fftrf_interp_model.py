"""A numpy restatement of FFTRF.interpolate (FFTRF.jl:107-129) as the device computes it (csrc/fftrf_points.hpp,
csrc/fftrf_interp.hip), and the case table of the tests.

Axis a of the field V (shape Ns, vec() index i0 + N0 (i1 + N1 i2)) belongs to row a of `points` (d x m).  Per axis
    lo, hi = min, max of that row over ALL m points (or the box);   step = (hi - lo) / (N - 1)
    t = (x - lo) / step;   t = min(max(t, 0), N - 1);   i = min(floor(t), N - 2);   f = t - i
and the value is the nested two-term sums (1 - f_a) A + f_a B, axis 0 innermost, the last axis outermost.  numpy rounds
every elementwise operation on its own, which is exactly what the planner (plain C++) and the kernel (contraction off) do:
`plan` and `interp` are compared with them bit for bit."""
import numpy as np

GRIDS = [(2, 2), (3, 5), (25, 37), (2, 3, 4), (6, 4, 5), (33, 2, 17)]
MODEL_GRIDS = GRIDS + [(4096, 2)]
POINT_COUNTS = [1, 63, 257, 1000]
FIELD_COUNTS = [1, 3, 131]


def gid(Ns):
    return "x".join(str(v) for v in Ns)


def extent(points, box=None):
    """(lo, hi) per axis: the points' extrema over all m points, or the box (lo of every axis, then hi)."""
    P = np.asarray(points, dtype=np.float64)
    d = P.shape[0]
    if box is None:
        return P.min(axis=1), P.max(axis=1)
    b = np.asarray(box, dtype=np.float64).reshape(-1)
    assert b.size == 2 * d
    return b[:d].copy(), b[d:].copy()


def plan(points, Ns, box=None, row0=0, rows=None):
    """base (int32, `rows`) and frac (d x rows) of the points [row0, row0 + rows); the extrema come from ALL points."""
    P = np.asarray(points, dtype=np.float64)
    d, m = P.shape
    assert d == len(Ns)
    rows = m - row0 if rows is None else rows
    lo, hi = extent(P, box)
    base = np.zeros(rows, dtype=np.int64)
    frac = np.empty((d, rows))
    stride = 1
    for a in range(d):
        N = int(Ns[a])
        step = (hi[a] - lo[a]) / np.float64(N - 1)
        t = (P[a, row0:row0 + rows] - lo[a]) / step
        t = np.minimum(np.maximum(t, 0.0), np.float64(N - 1))
        i = np.minimum(np.floor(t), np.float64(N - 2))
        frac[a] = t - i
        base += i.astype(np.int64) * stride
        stride *= N
    return base.astype(np.int32), frac


def interp(V, Ns, base, frac):
    """V: n x nf, column c = vec() of field c (or one field of shape Ns / length n) -> rows x nf."""
    V = np.asarray(V, dtype=np.float64)
    n = int(np.prod(Ns))
    V = V.reshape(n, 1, order="F") if V.shape == tuple(Ns) else V.reshape(n, -1)
    b = base.astype(np.int64)
    s1, s2 = int(Ns[0]), int(Ns[0]) * int(Ns[1])
    f = [frac[a][:, None] for a in range(len(Ns))]
    g = [1.0 - fa for fa in f]

    def line(b0):
        return g[0] * V[b0] + f[0] * V[b0 + 1]

    def plane(b0):
        return g[1] * line(b0) + f[1] * line(b0 + s1)

    if len(Ns) == 2:
        return plane(b)
    return g[2] * plane(b) + f[2] * plane(b + s2)


def interpolate(points, V, Ns, box=None, row0=0, rows=None):
    return interp(V, Ns, *plan(points, Ns, box, row0, rows))


# ---------------------------------------------------------------- inputs
def node_points(Ns, scale=1.0, shift=0.0):
    """The grid nodes in vec() order as d x n points with coordinates scale * index + shift."""
    idx = np.indices(Ns).reshape(len(Ns), -1, order="F").astype(np.float64)
    return idx * scale + shift


def scattered_points(Ns, m, seed=0):
    """m Gaussian points; from 4 points on: one duplicate, one point at the minimum of every axis, one at the maximum."""
    d = len(Ns)
    rng = np.random.default_rng([seed, m] + list(Ns))
    P = rng.standard_normal((d, m)) * np.arange(1, d + 1)[:, None] + 3.0
    if m >= 4:
        P[:, m // 2] = P[:, 0]
        lo, hi = P.min(axis=1), P.max(axis=1)
        P[:, 1] = lo
        P[:, m - 1] = hi
    return P


def inner_box(points, shrink=0.25):
    """A box inside the points' extent (so that the clamp acts), or around a single point."""
    P = np.asarray(points, dtype=np.float64)
    lo, hi = P.min(axis=1), P.max(axis=1)
    w = np.where(hi > lo, hi - lo, 1.0)
    if P.shape[1] == 1:
        return np.concatenate([lo - 0.3 * w, hi + 0.6 * w])
    return np.concatenate([lo + shrink * w, hi - 0.5 * shrink * w])


def random_fields(Ns, nf, seed=0):
    rng = np.random.default_rng([seed, nf] + list(Ns))
    return rng.standard_normal((int(np.prod(Ns)), nf))
