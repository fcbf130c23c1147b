"""A numpy model of the device FFTRF sampler (csrc/fftrf_sample.hip) and a reading of its launcher.

The model follows the device algorithm step by step -- per-axis unnormalised inverse DFT with the crop right behind it,
Bluestein's convolution of length P = next power of two >= 3 N - 1 wherever 2 N is not a power of two (chirp from the
INTEGER j^2 mod 2L), the reference's axis swap, the two-pass normalisation -- so that a disagreement between the device and
the oracle can be told apart from a disagreement between the ALGORITHM and the oracle.  `launches` says which kernel
instantiation each pass of a grid runs; `CASES` is the table the GPU test walks, and tests/test_fftrf_model.py asserts on
the CPU that it reaches every instantiation the launcher can produce."""
import numpy as np

FIRST, MIDDLE, LAST = "first", "middle", "last"


# ---------------------------------------------------------------- geometry (fftrf_geometry)
def geometry(Ns):
    """A = half lengths along the ARRAY axes (N_2, N_1[, N_3]), L = 2 A, per axis Bluestein or direct and the transform
    length P."""
    Ns = [int(v) for v in Ns]
    assert len(Ns) in (2, 3)
    A = [Ns[1], Ns[0]] + Ns[2:]
    L = [2 * a for a in A]
    blue = [(l & (l - 1)) != 0 for l in L]
    P = []
    for a, l, b in zip(A, L, blue):
        p = l
        if b:
            p = 1
            while p < l + a - 1:
                p <<= 1
        P.append(p)
    return A, L, blue, P


# ---------------------------------------------------------------- the launcher (frf_pass, fftrf_tile_lines, frf_launch_kb)
def tile_lines(Ma, contiguous, nl0):
    tpl = Ma // 16 if Ma >= 16 else 1
    T = 512 // tpl
    if contiguous:
        T = min(T, max(4096 // Ma, 1), 32)
    else:
        T = min(T, 16)
    return max(min(T, nl0), 1)


def launches(Ns):
    """One dict per pass: kind, Bluestein or direct, the transform length, the kernel's template arguments (last radix LR,
    short line), contiguous or strided, lines per tile and tiles per field."""
    A, L, blue, P = geometry(Ns)
    d = len(A)
    L3 = L + [1] * (3 - d)
    out = []
    for axis in range(d):
        Ma = P[axis]
        log2 = Ma.bit_length() - 1
        assert 1 << log2 == Ma and 2 <= Ma <= 8192
        short = Ma < 16
        if short and blue[axis]:
            assert Ma == 8
        lr = log2 if short else (log2 & 3)
        kind = FIRST if axis == 0 else (LAST if axis == d - 1 else MIDDLE)
        if axis == 0:
            nl0, nl1 = L3[1] * L3[2], 1
        elif axis == 1:
            nl0, nl1 = A[0], L3[2]
        else:
            nl0, nl1 = A[0], A[1]
        T = tile_lines(Ma, axis == 0, nl0)
        tpl = Ma // 16 if Ma >= 16 else 1
        threads = (T * tpl + 63) // 64 * 64
        assert threads <= 512 and T * Ma <= 8192
        out.append({"kind": kind, "bluestein": bool(blue[axis]), "length": Ma, "LR": lr, "short": short,
                    "contiguous": axis == 0, "lines_per_tile": T, "tiles": -(-nl0 // T) * nl1, "threads": threads})
    return out


def instantiation(launch):
    return (launch["kind"], launch["bluestein"], launch["LR"], launch["short"])


def all_instantiations():
    """Every fftrf_line_kernel<KIND, BLUE, LR, SHORT> the launcher can produce: short lines are direct lines of 2, 4 and 8
    points or the 8-point Bluestein line of N = 3."""
    out = set()
    for kind in (FIRST, MIDDLE, LAST):
        for lr in (1, 2, 3):
            out.add((kind, False, lr, True))
        out.add((kind, True, 3, True))
        for lr in (0, 1, 2, 3):
            out.add((kind, False, lr, False))
            out.add((kind, True, lr, False))
    return out


# ---------------------------------------------------------------- the algorithm
def chirp(L):
    j = np.arange(L, dtype=np.int64)
    r = (j * j) % (2 * L)                          # the integer j^2 mod 2L, then the division
    return np.exp(1j * np.pi * (r / L))


def _idft_crop_line_axis(x, axis, A, L, P, blue):
    """Unnormalised inverse DFT of length L along `axis`, first A outputs."""
    x = np.moveaxis(x, axis, -1)
    if not blue:
        y = np.fft.ifft(x, axis=-1) * L
        y = y[..., :A]
    else:
        c = chirp(L)
        b = np.zeros(P, dtype=complex)
        b[:A] = np.conj(c[:A])
        m = np.arange(1, L)
        b[P - m] = np.conj(c[m])
        bspec = np.fft.fft(b)
        a = np.zeros(x.shape[:-1] + (P,), dtype=complex)
        a[..., :L] = x * c
        conv = np.fft.ifft(np.fft.fft(a, axis=-1) * bspec, axis=-1)      # carries the 1 / P
        y = conv[..., :A] * c[:A]
    return np.moveaxis(y, -1, axis)


def sqrt_spectrum(Ns, beta):
    A, L, _, _ = geometry(Ns)
    S = np.zeros(L)
    for a, l in enumerate(L):
        k = np.arange(l)
        w = np.minimum(k, l - k).astype(float)
        shp = [1] * len(L)
        shp[a] = l
        S = S + (w ** 2).reshape(shp)
    out = np.zeros(L)
    nz = S > 0
    out[nz] = S[nz] ** (0.25 * beta)
    if beta == 0:
        out[~nz] = 1.0
    return out


def field(Ns, k0, dk, beta, phi, raw=False):
    """The device algorithm for one field; `phi` has the reference's size(S) = (2 N_2, 2 N_1[, 2 N_3])."""
    A, L, blue, P = geometry(Ns)
    phi = np.asarray(phi, dtype=np.float64)
    assert phi.shape == tuple(L)
    two_phi = 2.0 * phi
    red = two_phi - 2.0 * np.round(phi)            # exact argument reduction, as cospi / sinpi do it
    K = sqrt_spectrum(Ns, beta) * (np.cos(np.pi * red) + 1j * np.sin(np.pi * red))
    for axis in range(len(A)):
        K = _idft_crop_line_axis(K, axis, A[axis], L[axis], P[axis], blue[axis])
    f = K.real * (1.0 / float(np.prod(L)))
    f = np.swapaxes(f, 0, 1).copy()                # finalk[j, i, h] = real(k[i, j, h])
    if raw:
        return f
    n = f.size
    mean = f.sum() / n
    sd = np.sqrt(((f - mean) ** 2).sum() / (n - 1))
    return dk * (f - mean) / sd + k0


# ---------------------------------------------------------------- the oracle fed the same phi
class PhiStub:
    """Stands for the oracle's rng: `standard_normal(shape)` returns the phi it was given."""

    def __init__(self, phi):
        self.phi = np.asarray(phi, dtype=np.float64)

    def standard_normal(self, shape):
        assert tuple(shape) == self.phi.shape
        return self.phi


def oracle_field(Ns, k0, dk, beta, phi):
    from oracle import oracle as orc
    return orc.fftrf_powerlaw_structuredgrid(Ns, k0, dk, beta, PhiStub(phi))


def error_ratio(F, Fref, k0):
    """max |F - F_ref| / max |F_ref - k0|: what the bar of 1e-12 applies to."""
    return float(np.abs(F - Fref).max() / np.abs(Fref - k0).max())


BAR = 1e-12


# ---------------------------------------------------------------- the case table
class Case:
    def __init__(self, Ns, k0=0.0, dk=1.0, beta=-3.5, nfields=3, seed=None):
        self.Ns, self.k0, self.dk, self.beta, self.nfields = tuple(Ns), k0, dk, beta, nfields
        self.seed = seed if seed is not None else 1000 + sum((i + 1) * v for i, v in enumerate(Ns))

    @property
    def id(self):
        return "x".join(str(v) for v in self.Ns)

    def phi(self):
        _, L, _, _ = geometry(self.Ns)
        rng = np.random.default_rng(self.seed)
        return [rng.standard_normal(L) for _ in range(self.nfields)]


CASES = [
    # 2-D
    Case((25, 25), k0=2.0, dk=3.14), Case((4, 8)), Case((3, 5), beta=2.0), Case((3, 9)), Case((1, 7)), Case((16, 3), beta=0.0),
    Case((7, 11)), Case((33, 40)), Case((100, 37)), Case((300, 33), beta=-2.5), Case((6, 130)),
    # 2-D, long lines
    Case((3, 1000)), Case((1000, 3)), Case((2, 2048)), Case((2, 4096)), Case((2730, 2)), Case((600, 20)),
    # 3-D
    Case((6, 4, 5)), Case((2, 3, 4)), Case((5, 1, 3)), Case((17, 6, 4), beta=-4.0), Case((9, 130, 9)), Case((2, 300, 2)),
    Case((2, 2, 683)), Case((65, 2, 3)),
    # added until every instantiation is reached (tests/test_fftrf_model.py): direct lines of 16, 32, 64 and 128 points as the
    # first, a middle and the last pass; 2- and 8-point direct, 8-point and 128-point Bluestein lines as a middle pass
    Case((8, 32, 8)), Case((16, 64, 2)), Case((1, 2, 32)), Case((32, 2, 64)), Case((64, 3, 2)), Case((4, 5, 3)),
    Case((23, 2, 3)), Case((3, 2, 5)),
]
BATCH_CASE = Case((5, 3), nfields=131)
