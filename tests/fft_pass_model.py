"""A host model of how the FFT covariance operator launches its pass kernel, the case table of
test_fft_pass_kernels_gpu.py, and the exact integer reference of those cases.  No GPU, no library: plain arithmetic.

passes(Ns, l) mirrors, with every GSI_FFT_* knob at its default (GSI_FFT_TB=16, GSI_FFT_B0=64, GSI_FFT_B1=140,
GSI_FFT_MIN_T=4, GSI_FFT_LINE_SYNC=1, GSI_FFT_W_MB unset):

  csrc/hip_backend_products.hip  fftcov_new_plan  :132-140  singleton axes squeezed, M_a = next power of two >= 2 N_a
                                            :150-153  nb_max: pairs per batch, (256 MB | 2 GB) / (16 Mtot), at most 64
  csrc/fft_cov.hip      fft_cov_apply       :723-732  batches of nb_max pairs; d - 1 forward passes, the fused one, d - 1 back
                        fft_pass            :618-629  Ma, nin / nout, estride, R1 / R2 (the later axes, restricted)
                                            :631-652  the layout: lb, kind, OS
                                            :661-687  T and lstride (axis 0: :664-671, strided: :673-686)
                                            :691-697  threads, dynamic LDS, tiles, nitems
                                            :702-711  MODE
                        launch_pass         :603-608  LR = log2(Ma) mod 4, SHORT = Ma < 16
                        launch_pass_k       :591-592  G = min(ncus * per_cu, nitems)
                        fft_pass_kernel     :256-258  P, NPRE
                                            :280      wpl
                                            :291      s_lin
                                            :293-297  off(): uniform for R2 == 1, division otherwise
                                            :302      the XCD-permuted order when G % 8 == 0

What the occupancy API answers on the device is not modelled: `bound` is an upper bound on the resident workgroups per CU
(LDS and thread slots only), so `looping` (nitems > 256 * bound) holds whatever it answers, and `G` is given only where
it does not depend on it (nitems <= 256: per_cu >= 1 on a 256-CU chip)."""
import numpy as np

NCUS = 256                       # MI355X
LDS_LIMIT = 160 * 1024 - 64      # launch_pass_k: hipFuncAttributeMaxDynamicSharedMemorySize
FFT_MAX_TILE = 8192
MODES = (15, 3, 25, 4, 0, 16)    # AXIS0|LOADX|FUSED|STOREY (d = 1), AXIS0|LOADX, AXIS0|STOREY|INVERSE, FUSED, forward, INVERSE
AXIS0, FUSED, INVERSE = 1, 4, 16


def embed(N):
    m = 1
    while m < 2 * N:
        m <<= 1
    return 1 if N == 1 else m


def ilog2(v):
    r = 0
    while (1 << r) < v:
        r += 1
    return r


def _pass(N, M, d, axis, inverse, fused, nb, col0):
    Ma = M[axis]
    stride = (1, M[0], M[0] * M[1])
    estride = stride[axis]
    R1, R2 = 1, 1
    if axis == 0:
        R1, R2 = N[1], N[2]
    elif axis == 1:
        R1 = N[2]
    nouter = R1 * R2
    lb = 0
    if d >= 2 and M[0] >= 256:
        while (2 << lb) <= 16 and (2 << lb) <= 64 and (2 << lb) <= M[0] // 16:
            lb += 1
    Tb = 1 << lb
    kind, OS = 0, 0
    if lb > 0 and axis > 0:
        if axis == 1 and d == 3:
            kind, OS = 1, Tb
        elif axis == 1:
            kind, OS = 1, 0
        else:
            kind, OS = 2, N[2] * Tb
    line_bytes = Ma * 16
    tmax = FFT_MAX_TILE // Ma
    if axis == 0:
        T = min(64 * 1024 // line_bytes, tmax, 32, nouter)
        T = max(T, 1)
        lstride = Ma
    else:
        want = 140 * 1024 // line_bytes
        want = max(want, 4)
        want = min(want, 16, tmax, estride)
        if lb > 0:
            want = min(want, Tb, M[0])
        T = 1
        while 2 * T <= want:
            T *= 2
        lstride = Ma + (16 // T if T >= 2 else 0)
    tpl = Ma // 16 if Ma >= 16 else 1
    threads = (T * tpl + 63) // 64 * 64
    assert threads <= 512
    ntabB = Ma // 128 if Ma >= 128 else 1
    shmem = (64 + ntabB + T * lstride) * 16
    tiles = (nouter + T - 1) // T if axis == 0 else (estride // T) * nouter
    nitems = tiles * nb
    if axis == 0:
        mode = 15 if fused else (25 if inverse else 3)
    else:
        mode = 4 if fused else (16 if inverse else 0)
    L = ilog2(Ma)
    short = Ma < 16
    LR = L & 3
    assert not (short and LR == 0)
    P = (1 << LR) if short else 16
    NPRE = P if (mode & INVERSE) else P // 2
    bound = max(1, min(LDS_LIMIT // shmem, 2048 // threads))
    return dict(axis=axis, mode=mode, inst=(mode, LR, short), Ma=Ma, T=T, threads=threads, lb=lb, kind=kind, OS=OS,
                s_lin=(None if axis == 0 else (threads // T) * NPRE <= Ma), wpl=(tpl >> 6 if tpl >= 64 else 1),
                ragged=(nouter % T != 0 if axis == 0 else None), off_form=("uniform" if R2 == 1 else "division"),
                nb=nb, col0=col0, tiles=tiles, nitems=nitems, shmem=shmem, bound=bound, looping=nitems > NCUS * bound,
                G=(nitems if nitems <= NCUS else None))


def passes(Ns, l):
    """One dict per fft_pass_kernel launch of one product with l columns on the grid Ns, in launch order."""
    N = [int(v) for v in Ns if int(v) != 1]
    d = len(N)
    assert 1 <= d <= 3
    N += [1] * (3 - d)
    M = [embed(v) for v in N]
    Mtot = M[0] * M[1] * M[2]
    assert max(M) <= 8192 and Mtot < 2 ** 31
    w_mb = 256 if (d == 2 and 16 * Mtot <= (128 << 20)) else 2048
    nb_max = max(1, min((w_mb << 20) // (16 * Mtot), 64))
    npairs = (l + 1) // 2
    out = []
    for p0 in range(0, npairs, nb_max):
        nb = min(npairs - p0, nb_max)
        for a in range(d - 1):
            out.append(_pass(N, M, d, a, False, False, nb, 2 * p0))
        out.append(_pass(N, M, d, d - 1, False, True, nb, 2 * p0))
        for a in range(d - 2, -1, -1):
            out.append(_pass(N, M, d, a, True, False, nb, 2 * p0))
    return out


def inst_name(inst):
    """The kernel's name as profiles/isa_resources.json spells it."""
    return "gsi::hipk::fft_pass_kernel<%d, %d, %s>" % (inst[0], inst[1], "true" if inst[2] else "false")


# ---- the case table of test_fft_pass_kernels_gpu.py: (Ns, l) ---------------------------------------------------------------
CASES_1D = [((2,), 1), ((3,), 2), ((4,), 3), ((7,), 3), ((13,), 2), ((31,), 5), ((50,), 7), ((100,), 3), ((200,), 2),
            ((300,), 3), ((600,), 131), ((1500,), 3), ((4096,), 3)]
CASES_2D_NATURAL = [((2, 5), 3), ((3, 9), 2), ((5, 2), 3), ((9, 3), 5), ((17, 17), 131), ((33, 40), 7), ((4, 70), 3),
                    ((6, 130), 2), ((3, 1100), 3), ((2, 2049), 2), ((5, 600), 3)]
CASES_2D_BLOCKED = [((65, 2), 3), ((130, 7), 5), ((300, 3), 2), ((600, 20), 3), ((1100, 3), 1), ((2049, 2), 3),
                    ((70, 300), 19), ((66, 600), 1), ((300, 33), 131), ((2049, 9), 59)]
CASES_3D_NATURAL = [((3, 2, 5), 3), ((5, 3, 2), 2), ((2, 5, 9), 3), ((4, 9, 3), 3), ((6, 17, 4), 5), ((3, 40, 5), 2), ((3, 70, 5), 3),
                    ((9, 6, 11), 131), ((2, 130, 3), 2), ((2, 300, 2), 1), ((2, 600, 2), 2), ((2, 1100, 2), 1),
                    ((9, 130, 9), 29)]
CASES_3D_BLOCKED = [((65, 2, 3), 3), ((130, 3, 5), 2), ((70, 5, 9), 3), ((66, 9, 17), 2), ((65, 17, 2), 3), ((70, 40, 3), 2),
                    ((65, 130, 2), 1), ((65, 300, 2), 2), ((65, 3, 40), 2), ((65, 2, 130), 1), ((130, 40, 3), 67)]
CASES = CASES_1D + CASES_2D_NATURAL + CASES_2D_BLOCKED + CASES_3D_NATURAL + CASES_3D_BLOCKED
BLOCKED_CASES = CASES_2D_BLOCKED + CASES_3D_BLOCKED


def case_id(case):
    Ns, l = case
    return "x".join(str(v) for v in Ns) + "-l%d" % l


# ---- inputs and the exact reference --------------------------------------------------------------------------------------
def int_table(Ns):
    """Integer lag table in [-3, 3], seeded from Ns: tab[t0, t1, t2] = c(t), t >= 0."""
    seed = [len(Ns)] + [int(v) for v in Ns]
    return np.random.default_rng(seed).integers(-3, 4, size=tuple(Ns)).astype(np.float64)


def int_panel(Ns, l):
    """X (n x l, Fortran order) with integer entries in [-4, 4]."""
    n = int(np.prod(Ns))
    rng = np.random.default_rng([l] + [int(v) for v in Ns])
    return np.asfortranarray(rng.integers(-4, 5, size=(n, l)).astype(np.float64))


def dense_reference(tab, X):
    """A X with A[i, j] = tab[|i0 - j0|, |i1 - j1|, |i2 - j2|] built by index arithmetic (points in column-major order).
    Exact: integer entries, every partial sum an integer far below 2^53."""
    Ns = tab.shape
    idx = np.unravel_index(np.arange(int(np.prod(Ns))), Ns, order="F")
    A = tab[tuple(np.abs(ia[:, None] - ia[None, :]) for ia in idx)]
    return A @ X


def _toeplitz(c):
    i = np.arange(len(c))
    return c[np.abs(i[:, None] - i[None, :])]


def structured_reference(tab, X):
    """The same product by the block-Toeplitz structure: for each lag (t1, t2) along the later axes the dense axis-0 Toeplitz
    block times the matching slab of X, shift-added.  Nothing of size n^2 exists.  Exact for the same reason."""
    Ns = tuple(tab.shape) + (1,) * (3 - tab.ndim)
    N0, N1, N2 = Ns
    l = X.shape[1]
    tab3 = tab.reshape(Ns)
    X4 = np.asarray(X).reshape((N0, N1, N2, l), order="F")
    Xm = np.ascontiguousarray(X4).reshape(N0, N1 * N2 * l)
    Y4 = np.zeros((N0, N1, N2, l))
    for a1 in range(N1):
        for a2 in range(N2):
            Z = (_toeplitz(tab3[:, a1, a2]) @ Xm).reshape(N0, N1, N2, l)        # Z[:, j1, j2] = T0(a1, a2) X[:, j1, j2]
            for s1 in ((a1, -a1) if a1 else (0,)):                              # i1 = j1 + s1
                for s2 in ((a2, -a2) if a2 else (0,)):
                    d1, d2 = slice(max(s1, 0), N1 + min(s1, 0)), slice(max(s2, 0), N2 + min(s2, 0))
                    f1, f2 = slice(max(-s1, 0), N1 + min(-s1, 0)), slice(max(-s2, 0), N2 + min(-s2, 0))
                    Y4[:, d1, d2] += Z[:, f1, f2]
    return np.asfortranarray(Y4.reshape((N0 * N1 * N2, l), order="F"))


def exact_reference(tab, X):
    Y = dense_reference(tab, X) if tab.size <= 4096 else structured_reference(tab, X)
    assert np.abs(Y).max() < 2.0 ** 50
    return Y


def host_fft_product(tab, X):
    """The same embedding through numpy's double-precision FFT: the kernel on the periodic grid of M_a points (zero beyond
    the lags of the box), its spectrum, and pad / transform / multiply / transform back / restrict per column."""
    Ns = tab.shape
    Ms = [embed(N) for N in Ns]
    c = np.zeros(Ms)
    for signs in np.ndindex(*(2,) * len(Ns)):
        src = tuple(slice(1, N) if s else slice(0, N) for s, N in zip(signs, Ns))
        dst = tuple(slice(M - 1, M - N, -1) if s else slice(0, N) for s, N, M in zip(signs, Ns, Ms))
        c[dst] = tab[src]
    lam = np.fft.fftn(c).real
    box = tuple(slice(0, N) for N in Ns)
    axes = tuple(range(len(Ns)))
    Y = np.empty_like(X)
    for j0 in range(0, X.shape[1], 8):                      # a few columns at a time: the padded array stays small
        Xc = X[:, j0:j0 + 8]
        w = np.zeros(tuple(Ms) + (Xc.shape[1],))
        w[box] = Xc.reshape(tuple(Ns) + (Xc.shape[1],), order="F")
        y = np.fft.ifftn(np.fft.fftn(w, axes=axes) * lam[..., None], axes=axes).real
        Y[:, j0:j0 + 8] = y[box].reshape((-1, Xc.shape[1]), order="F")
    return Y
