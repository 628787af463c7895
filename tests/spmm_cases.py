"""Patterns, float64 reference, data sets, error bounds, the instantiation table and a numpy
emulation of the plan-based SpMM (bsmr_spmm / bsmr_spmm_t, the SDDMM gradients). No GPU here:
tests/test_spmm_ref_cpu.py checks this module; tests/test_gpu_spmm.py, test_gpu_spmm_float64.py,
test_gpu_spmm_edges.py and test_gpu_autograd.py use it.

Reference: spmm_ref, numpy float64 straight from the CSR on the operands as the kernel sees them.

Data:
  * grid (grid_values for V, sddmm_cases.grid_data for X): multiples of 1/8 in [-4, 4). Every
    product is a multiple of 2^-6 of magnitude <= 16, so every partial sum of n < 2^14 products is
    a multiple of 2^-6 below 2^18: at most 24 bits. Y is therefore exact in fp32 whatever the
    chunk, lane group, butterfly or reduce order, for every list of this suite (n <= 2048), and
    the tests demand Y == ref bit for bit: a dropped, doubled or misindexed term, a wrong vpos or
    a skipped partial row fails with no tolerance.
  * signed (signed_values for V, sddmm_cases.signed_data for X): full-mantissa fp32, held to
    signed_bound_tight.

Bounds per element, n the destination's list length, S = sum |v x|:
  * signed_bound: 2 n 2^-24 S + 1e-6, the deterministic bound of an n-term fp32 sum of
    once-rounded products in any order (the older tests);
  * signed_bound_tight: min(2 n, 8 sqrt n) 2^-24 S + 1e-6 scale, the forward tests' two regimes
    (sddmm_cases.sddmm_bound) with n in place of K: the deterministic bound and the Higham-Mary
    probabilistic bound with lambda = 8, whichever is smaller. Derived, never widened from what
    a GPU shows.

SPMM_CASES: one (K, dtype) row per kernel instantiation and per generic lane count / tile count.
The instantiation is a pure function of (rowBytes, dtype) (csrc/spmm.hip pick_spmm / launch_side,
restated by spmm_form), with no fall-back between them, so (K, dtype) is the evidence:

  fixed, k_spmm<DT, LANES, CH>, for DT in f32 (K = rowBytes / 4), f16 and bf16 (K = rowBytes / 2):
    128 B  <DT, 8, 1>   f32 K = 32,  half K = 64        1 KiB  <DT, 64, 1>  f32 K = 256, half K = 512
    256 B  <DT, 16, 1>  f32 K = 64,  half K = 128       2 KiB  <DT, 64, 2>  f32 K = 512, half K = 1024
    512 B  <DT, 32, 1>  f32 K = 128, half K = 256
  generic, k_spmm<DT, 0, 1> with a.lanes = L (lanes past the row idle, 1-KiB column tiles):
    32 B    L = 2               half K = 16
    64 B    L = 4               f32 K = 16, half K = 32
    96 B    L = 8, 6 live       half K = 48
    192 B   L = 16, 12 live     f32 K = 48, half K = 96
    384 B   L = 32, 24 live     f32 K = 96, half K = 192
    768 B   L = 64, 48 live     f32 K = 192, half K = 384
    1280 B  2 tiles (64 + 16)   f32 K = 320, half K = 640
    3072 B  3 full tiles        f32 K = 768, half K = 1536
    4096 B  4 full tiles        f32 K = 1024

spmm_emulate restates the documented summation order in numpy fp32 over the
library's own host lists, with the mutations test_spmm_ref_cpu.py uses to show that the checks
reject a subtly wrong kernel.
"""
import functools

import numpy as np

import bsmr
from bsmr import BF16, F16, F32, synth

SPMM_DIRECT = bsmr.SPMM_DIRECT
DEFAULT_CHUNK = 128  # csrc/spmm_schedule.hpp SPMM_CHUNK_DEFAULT (what chunk = 0 builds on a fresh plan)
DTYPE_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}


def shuffled(pattern, seed=7):
    """The same pattern with the columns of every CSR row in random ("file") order."""
    M, N, rp, ci = pattern
    rng = np.random.default_rng(seed)
    ci = ci.copy()
    for r in range(M):
        rng.shuffle(ci[rp[r]:rp[r + 1]])
    return M, N, rp, ci


def _staircase(n=272):
    """Entry (i, j) stored iff j < i: row i holds i entries, column j holds n - 1 - j."""
    lens = np.arange(n, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    ci = np.concatenate([np.arange(i, dtype=np.uint32) for i in range(n)])
    return n, n, rp, ci


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
    if name == "staircase":  # 36,856 entries; both sides see every list length 0 .. 271
        return _staircase()
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


def signed_bound_tight(S, n, scale=1.0):
    """|Y - ref| <= min(2 n, 8 sqrt n) 2^-24 S + 1e-6 scale per element (module docstring);
    `scale` is the product of the operand scalings."""
    n = np.asarray(n, np.float64)[:, None]
    return np.minimum(2.0 * n, 8.0 * np.sqrt(n)) * 2.0 ** -24 * np.asarray(S, np.float64) + 1e-6 * scale


def grid_values(nnz, seed):
    """nnz fp32 values k / 8, k a non-zero integer in [-32, 32): sddmm_cases.grid_data with its
    zeros (one value in 64) moved to -4, so that every stored entry contributes and a dropped or
    doubled term changes its destination. With X from grid_data every product is a multiple of
    2^-6 of magnitude <= 16 and any partial sum of n < 2^14 of them fits in 24 bits: Y is exact
    in fp32 in every summation order, for every list of this suite (n <= 2048)."""
    from sddmm_cases import grid_data
    V = grid_data(nnz, seed)
    V[V == 0] = np.float32(-4.0)
    return V


def signed_values(nnz, seed):
    """nnz fp32 values +-(0.5 + u), u uniform in [0, 1) (full mantissa). No value is near zero:
    a single dropped term |v x| then stands far above signed_bound_tight in at least one column,
    which a standard normal V (one value in 10^3 below 10^-3) does not guarantee."""
    rng = np.random.default_rng(seed)
    mag = np.float32(0.5) + rng.random(int(nnz), dtype=np.float32)
    return np.where(rng.integers(0, 2, int(nnz)) == 1, mag, -mag).astype(np.float32)


def bound_ratio(Y, ref, scale=1.0):
    """max over elements of |Y - ref| / signed_bound_tight (inf where Y is not finite)."""
    Yr, S, n = ref
    r = np.abs(np.asarray(Y, np.float64) - Yr) / signed_bound_tight(S, n, scale)
    return float(np.where(np.isfinite(r), r, np.inf).max()) if r.size else 0.0


def assert_exact(Y, ref, what):
    """Y (fp32) equals the exact float64 reference bit for bit, every element written, empty
    destinations exactly 0."""
    Yr, _, n = ref
    assert Y.dtype == np.float32 and Y.shape == Yr.shape, (what, Y.dtype, Y.shape)
    assert np.isfinite(Y).all(), f"{what}: {int((~np.isfinite(Y)).sum())} elements never written"
    assert (Y[n == 0] == 0).all(), f"{what}: an empty destination is not exactly 0"
    bad = np.nonzero((Y.astype(np.float64) != Yr).any(axis=1))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(Y)} destinations differ from the exact result, "
                           f"first {bad[:5]} (lists of {n[bad[:5]]}): got {Y[bad[0], :4]} want {Yr[bad[0], :4]}")


def assert_tight(Y, ref, what, kind, scale=1.0):
    """Y within signed_bound_tight of the reference, every element written, empty destinations
    exactly 0; prints "RATIO spmm/kind x what"."""
    _, _, n = ref
    assert np.isfinite(Y).all(), f"{what}: {int((~np.isfinite(Y)).sum())} elements never written"
    assert (Y[n == 0] == 0).all(), f"{what}: an empty destination is not exactly 0"
    ratio = bound_ratio(Y, ref, scale)
    print(f"RATIO spmm/{kind} {ratio:.4f} {what}")
    assert ratio <= 1.0, f"{what}: worst |Y - ref| / bound = {ratio:.3f}"


def list_lengths(pat, side):
    """Entries per destination: rows (side 1) or columns (side 2)."""
    M, N, rp, ci = pat
    return np.diff(np.asarray(rp, np.int64)) if side == 1 else np.bincount(ci, minlength=N)


def expected_stats(pat, side, chunk):
    """Plan.spmm_stats(side) as the list lengths give it: every destination has
    max(1, ceil(len / chunk)) segments, one of several writes one partial row per segment."""
    lens = list_lengths(pat, side)
    nseg = np.maximum(1, -(-lens // chunk))
    return dict(segments=int(nseg.sum()), split_dsts=int((nseg > 1).sum()),
                partials=int(nseg[nseg > 1].sum()), max_list=int(lens.max()), chunk=int(chunk))


def row_bytes(K, dtype):
    return K * (4 if dtype == F32 else 2)


def spmm_form(K, dtype):
    """csrc/spmm.hip pick_spmm / launch_side restated: dict(fixed, lanes, ch, live, tiles) of the
    instantiation a launch at (K, dtype) runs. fixed: k_spmm<DT, lanes, ch>; else the generic
    k_spmm<DT, 0, 1> with a.lanes = lanes, of which `live` hold a chunk in the last column tile."""
    rb = row_bytes(K, dtype)
    assert K > 0 and K % 16 == 0
    chunks = rb // 16
    if rb in (128, 256, 512, 1024, 2048):
        lanes = min(64, chunks)
        return dict(fixed=True, lanes=lanes, ch=chunks // lanes, live=lanes, tiles=1)
    lanes = 1
    while lanes < chunks and lanes < 64:
        lanes <<= 1
    tiles = -(-chunks // 64)
    return dict(fixed=False, lanes=lanes, ch=1, live=chunks - 64 * (tiles - 1), tiles=tiles)


def _spmm_cases():
    out = []
    for rb in (128, 256, 512, 1024, 2048):  # the 15 fixed instantiations
        out += [(rb // 4, F32), (rb // 2, F16), (rb // 2, BF16)]
    for rb in (32, 64, 96, 192, 384, 768, 1280, 3072, 4096):  # the generic form (module docstring)
        if rb % 64 == 0:
            out.append((rb // 4, F32))
        if rb < 4096:  # (the largest half row of the suite is 3072 B)
            out += [(rb // 2, F16), (rb // 2, BF16)]
    assert len(set(out)) == len(out)
    return out


SPMM_CASES = _spmm_cases()


def case_id(K, dtype):
    return f"K{K}_{DTYPE_NAME[dtype]}"


MUTATIONS = ("drop_last", "double_first", "vpos_shift", "skip_last_partial", "round_bf16")


def spmm_emulate(pat, side, chunk, V, X, rowBytes, mutation=None):
    """Y (fp32, destinations x X.shape[1]) as k_spmm / k_spmm_reduce sum it (DESIGN.md section
    11), in numpy over the library's own host lists (bsmr.spmm_lists, no GPU):
      * a segment's row is covered by L = rowBytes / 16 lanes rounded up to a power of two (at
        most 64: a longer row goes in column tiles of the same order), so G = 64 / L lane groups
        work at once; group g takes entries g, g + G, ... of the segment in order, one FMA (one
        rounding) per term;
      * the groups are added by the xor butterfly with offsets 32 .. L (G / 2 .. 1 in groups);
      * a destination of several segments adds its partial rows in chunk order.
    The FMA is a float64 product (exact for fp32 factors) and sum rounded to fp32, which differs
    from one rounding only in rare double-rounding ties. The order depends on rowBytes alone, so
    X may hold any number of columns. mutation (MUTATIONS): a wrong kernel, for
    test_spmm_ref_cpu.py: "drop_last": every segment loses its last entry; "double_first": every
    segment but a destination's last also takes the next one's first entry (an overlapping chunk
    boundary); "vpos_shift": entry k of a list takes the value of entry k + 1 (the last takes the
    first's); "skip_last_partial": the reduce leaves out a split destination's last partial row;
    "round_bf16": the result is rounded to bf16."""
    assert mutation is None or mutation in MUTATIONS, mutation
    M, N, rp, ci = pat
    D = M if side == 1 else N
    V = np.asarray(V, np.float32)
    X = np.asarray(X, np.float32)
    K = X.shape[1]
    segs, src, vpos = bsmr.spmm_lists(M, N, rp, ci, side, chunk)
    dst, first, count, part = (segs[:, i].astype(np.int64) for i in range(4))
    nS = len(segs)
    split = part != SPMM_DIRECT
    # a split destination's segments are consecutive; rank: a segment's place among them
    rank = np.zeros(nS, np.int64)
    if split.any():
        part0 = np.full(D, np.iinfo(np.int64).max)
        sp = np.nonzero(split)[0]
        np.minimum.at(part0, dst[sp], part[sp])  # a destination's first partial slot
        rank[sp] = part[sp] - part0[dst[sp]]
    last = np.ones(nS, bool)  # the destination's last segment
    last[:-1] = dst[1:] != dst[:-1]
    src = src.astype(np.int64)
    vpos = vpos.astype(np.int64)
    if mutation == "drop_last":
        count = np.maximum(count - 1, 0)
    elif mutation == "double_first":
        count = count + (~last)
    elif mutation == "vpos_shift":
        lens = list_lengths(pat, side)
        start = np.cumsum(lens) - lens
        k = np.arange(len(vpos)) - np.repeat(start, lens)
        vpos = vpos[np.repeat(start, lens) + (k + 1) % np.repeat(np.maximum(lens, 1), lens)]

    chunks16 = rowBytes // 16
    L = 1
    while L < chunks16 and L < 64:
        L <<= 1
    G = 64 // L
    acc = np.zeros((nS, G, K), np.float32)
    for t in range(-(-int(count.max(initial=0)) // G)):
        for g in range(G):
            s = np.nonzero(count > t * G + g)[0]
            if len(s) == 0:
                break
            e = first[s] + t * G + g
            term = V[vpos[e]].astype(np.float64)[:, None] * X[src[e]]
            acc[s, g] = (term + acc[s, g]).astype(np.float32)
    lanes = np.arange(G)
    o = G // 2
    while o >= 1:
        acc = acc + acc[:, lanes ^ o]
        o //= 2
    rows = acc[:, 0]

    Y = np.full((D, K), np.nan, np.float32)
    Y[dst[~split]] = rows[~split]
    for r in range(int(rank.max(initial=0)) + 1 if split.any() else 0):
        s = np.nonzero(split & (rank == r))[0]
        if mutation == "skip_last_partial":
            s = s[~last[s]]
        Y[dst[s]] = rows[s] if r == 0 else Y[dst[s]] + rows[s]
    if mutation == "round_bf16":
        from gpu_util import half_values
        Y = half_values(Y, BF16)
    return Y


def mutation_touches(pat, side, chunk, V, ref, mutation):
    """Destinations (bool mask) whose result a mutation of spmm_emulate changes, from the lists
    and the data alone: drop_last: every non-empty list (no V is 0); double_first and
    skip_last_partial: every list longer than `chunk`; vpos_shift: every list in which the shift
    gives some entry another value; round_bf16: every destination whose exact result (ref[0])
    holds an element that bf16 cannot."""
    lens = list_lengths(pat, side)
    if mutation == "drop_last":
        return lens > 0
    if mutation in ("double_first", "skip_last_partial"):
        return lens > chunk
    if mutation == "vpos_shift":
        M, N, rp, ci = pat
        _, _, vpos = bsmr.spmm_lists(M, N, rp, ci, side, chunk)
        v = np.asarray(V)[vpos.astype(np.int64)]
        start = np.cumsum(lens) - lens
        k = np.arange(len(v)) - np.repeat(start, lens)
        nxt = v[np.repeat(start, lens) + (k + 1) % np.repeat(np.maximum(lens, 1), lens)]
        return np.bincount(np.repeat(np.arange(len(lens)), lens), weights=(nxt != v), minlength=len(lens)) > 0
    if mutation == "round_bf16":
        from gpu_util import half_values
        Yr = ref[0]
        return (half_values(Yr.astype(np.float32), BF16).astype(np.float64) != Yr).any(axis=1)
    raise KeyError(mutation)
