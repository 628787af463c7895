"""Patterns and float64 references shared by the SpMM / SDDMM-gradient tests."""
import functools

import numpy as np

from bsmr import synth


def shuffled(pattern, seed=7):
    """The same pattern with the columns of every CSR row in random ("file") order."""
    M, N, rp, ci = pattern
    rng = np.random.default_rng(seed)
    ci = ci.copy()
    for r in range(M):
        rng.shuffle(ci[rp[r]:rp[r + 1]])
    return M, N, rp, ci


def _hub():
    counts = np.random.default_rng(5).integers(1, 4, 67)
    counts[3] = 2048
    return synth.random_rows(67, 2048, counts, seed=5)


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(M, N, rowptr, colidx), built once per process; callers do not modify the arrays."""
    if name == "zipf":  # 31,170 entries, M % 16 != 0, longest column 517, 619 empty columns
        return synth.random_rows(517, 4000, 60, seed=2, zipf=1.1)
    if name == "empty":  # 69 empty rows, 260 empty columns
        return synth.random_rows(300, 900, 5, seed=3, empty_frac=0.2)
    if name == "hub":  # one row holds every column, the others 1-3
        return _hub()
    if name == "zipf_shuffled":
        return shuffled(pattern("zipf"))
    raise KeyError(name)


PATTERNS = ["zipf", "empty", "hub", "zipf_shuffled"]


def entry_rows(M, rp):
    return np.repeat(np.arange(M, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))


def spmm_ref(pat, side, V, X):
    """float64 (Y, sum of |v x| per element, list length per destination) of Y = S(V) X (side 1,
    X = B) or S(V)^T X (side 2, X = A), straight from the CSR."""
    M, N, rp, ci = pat
    rows = entry_rows(M, rp)
    cols = np.asarray(ci, np.int64)
    dst, src, D = (rows, cols, M) if side == 1 else (cols, rows, N)
    V = np.asarray(V, np.float64)
    X = np.asarray(X, np.float64)
    n = np.bincount(dst, minlength=D)
    by_dst = np.argsort(dst, kind="stable")
    live = np.nonzero(n)[0]
    starts = (np.cumsum(n) - n)[live]
    Y = np.zeros((D, X.shape[1]))
    S = np.zeros_like(Y)
    for k0 in range(0, X.shape[1], 256):  # column blocks bound the temporaries
        terms = V[by_dst, None] * X[src[by_dst], k0:k0 + 256]
        Y[live, k0:k0 + 256] = np.add.reduceat(terms, starts, axis=0)
        S[live, k0:k0 + 256] = np.add.reduceat(np.abs(terms), starts, axis=0)
    return Y, S, n


def signed_bound(S, n):
    """|Y - ref| <= 2 n 2^-24 sum|v x| + 1e-6: an n-term fp32 sum of once-rounded products."""
    return 2.0 * n[:, None] * 2.0 ** -24 * S + 1e-6
