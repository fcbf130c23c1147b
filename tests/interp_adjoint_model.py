"""A numpy restatement of the adjoint of FFTRF.interpolate -- the spread G = W' X of csrc/interp_adjoint.hip -- and of the
inverted index it walks (csrc/interp_adjoint_plan.hpp).  `base`, `frac` come from `fftrf_interp_model.plan`.

Point p reaches the 2^d nodes  g = base[p] + (k & 1) + (k >> 1 & 1) N0 + (k >> 2 & 1) N0 N1,  k = the corner code, with weight
prod_a (f_a if bit a of k else 1 - f_a).  The index lists, per node, its (point, corner) pairs in ascending point order; a
list of more than `chunk` pairs is cut into chunks of exactly `chunk` pairs and one shorter remainder."""
import numpy as np


def corner_offsets(Ns):
    d = len(Ns)
    s = [1, int(Ns[0]), int(Ns[0]) * int(Ns[1])]
    return np.array([sum(((k >> a) & 1) * s[a] for a in range(d)) for k in range(1 << d)], dtype=np.int64)


def corner_weights(frac, dtype=np.float64):
    """m x 2^d: the weight of every corner; axis 0 first, every product rounded on its own (as the kernel does)."""
    d, m = frac.shape
    f = frac.astype(dtype)
    W = np.empty((m, 1 << d), dtype=dtype)
    for k in range(1 << d):
        w = f[0] if k & 1 else 1 - f[0]
        for a in range(1, d):
            w = w * (f[a] if (k >> a) & 1 else 1 - f[a])
        W[:, k] = w
    return W


def index(base, Ns, chunk):
    """The inverted index as a dict of the arrays of csrc/interp_adjoint_plan.hpp."""
    n, m, nc = int(np.prod(Ns)), len(base), 1 << len(Ns)
    nodes = (base.astype(np.int64)[:, None] + corner_offsets(Ns)[None, :]).reshape(-1)      # contribution p * nc + k
    order = np.argsort(nodes, kind="stable")                                                # stable: ascending point per node
    counts = np.bincount(nodes, minlength=n)
    nodeptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    long_node = np.nonzero(counts > chunk)[0]
    chunk_off, chunk_len, long_chunk0 = [], [], [0]
    for g in long_node:
        b, ln = int(nodeptr[g]), int(counts[g])
        for o in range(0, ln, chunk):
            chunk_off.append(b + o)
            chunk_len.append(min(chunk, ln - o))
        long_chunk0.append(len(chunk_off))
    return {"n": n, "m": m, "chunk": int(chunk), "maxlen": int(counts.max()) if n else 0, "nodeptr": nodeptr,
            "point": (order // nc).astype(np.int32), "corner": (order % nc).astype(np.uint8),
            "long_node": long_node.astype(np.int32), "long_chunk0": np.array(long_chunk0, dtype=np.int64),
            "chunk_off": np.array(chunk_off, dtype=np.int64), "chunk_len": np.array(chunk_len, dtype=np.int32)}


def spread(X, Ns, base, frac, absolute=False):
    """G = W' X in np.longdouble (n x nf); absolute: sum of |w| |x| instead, the scale of the rounding bounds."""
    X = np.asarray(X, dtype=np.float64)
    X = X.reshape(X.shape[0], -1)
    n = int(np.prod(Ns))
    W = corner_weights(frac, np.longdouble)
    Xl = X.astype(np.longdouble)
    if absolute:
        W, Xl = np.abs(W), np.abs(Xl)
    nodes = base.astype(np.int64)[:, None] + corner_offsets(Ns)[None, :]
    G = np.zeros((n, X.shape[1]), dtype=np.longdouble)
    for k in range(W.shape[1]):
        np.add.at(G, nodes[:, k], W[:, k, None] * Xl)
    return G


def node_counts(base, Ns):
    """k_g: contributions per node."""
    nodes = (base.astype(np.int64)[:, None] + corner_offsets(Ns)[None, :]).reshape(-1)
    return np.bincount(nodes, minlength=int(np.prod(Ns)))


def weights_matrix(Ns, base, frac):
    """The dense m x n interpolation matrix W (float64)."""
    m, n = len(base), int(np.prod(Ns))
    W = np.zeros((m, n))
    cw = corner_weights(frac)
    nodes = base.astype(np.int64)[:, None] + corner_offsets(Ns)[None, :]
    W[np.arange(m)[:, None], nodes] = cw
    return W


# ---------------------------------------------------------------- the sampler comparison (tests 8 of test_fft_at_gpu.py)
SAMPLER_SEED = 5          # numpy seed of the noise handed to the sampler: the CPU test confirms the bound for it on the model
SAMPLER_N = 2048          # fields


def sampler_case():
    """32 x 32 exponential grid (ell = 6), 40 fixed points inside it, unit steps."""
    Ns = (32, 32)
    P = 31.0 * np.random.default_rng(53).random((2, 40))
    box = np.array([0.0, 0.0, 31.0, 31.0])
    return Ns, P, box


def sampler_noise(mtot):
    """Mtot x SAMPLER_N: column c the N(0, 1) noise of role c (gridcov_sample_model.fields_from_eps, GridCovSampler.fields)."""
    return np.asfortranarray(np.random.default_rng(SAMPLER_SEED).standard_normal((mtot, SAMPLER_N)))


def sampler_bound(sigma2=1.0, nugget=0.0):
    """6 sqrt(2 / N) (sigma2 + nugget): an entry's Monte-Carlo standard deviation is at most sqrt(2 / N) sigma2."""
    return 6.0 * np.sqrt(2.0 / SAMPLER_N) * (sigma2 + nugget)
