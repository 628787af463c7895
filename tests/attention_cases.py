"""Patterns, float64 reference, data sets, bounds and a numpy-fp32 emulation of the fused sparse
attention forward (bsmr_attention). No GPU here: tests/test_attention_ref_cpu.py
checks this module; test_gpu_attention_fused_float64.py, test_gpu_attention_fused_edges.py and
test_gpu_attention_fused_autograd.py use it.

Reference: attention_ref, numpy float64 straight from the CSR on the operands as the kernel sees
them (fp16 / bf16 rounded on the host): per entry the score p and S = sum_k |q k|, the weight W,
per row O, LSE = m scale + ln l, and what the bounds need.

Data:
  * selector (exact): Q[:, 0] = 1, every other Q column 0; K[j, 0] = 1000 (pi(j) + 1) for a
    permutation pi of the columns, the other K columns signed junk (multiplied by 0); V signed.
    A score is 1000 (pi(j) + 1) exactly, so per row the entry with the largest pi wins by at least
    1000 scale >= 125, every other weight underflows to exactly 0, l = 1 and 1 / l = 1:
    O[i, :] = V[j*(i), :] bit for bit and LSE[i] = scale 1000 (pi(j*) + 1) exactly (scale a power of
    two). fp16 / bf16 cannot hold 1000 (pi + 1); there the same score, with 1024 for 1000, is the
    exact fp32 sum of two exact products (selector). pi random, ascending in j (with sorted rows
    the maximum grows in every segment and the winner is the row's last entry) or descending (the
    winner is the first);
  * signed: Q, K, V uniform in [-1, 1) (full mantissa), Q scaled so that |p scale| reaches about 1
    (narrow) or about 8 (wide), held to attention_bound.

attention_bound, per element of O, with u = 2^-24, n the row length, d_e = (p_e - m) scale:
    |O_k - ref| <= sum_e dW_e |V_ek| + (min(n, 8 sqrt n) + 2) u sum_e W_e |V_ek|
    dW_e = W_e 2 scale max_e |dp| + W_e (C + 3 |d_e| + 3 sum_i W_i |d_i| + min(n, 8 sqrt n)) u + 2^-125
  * |dp_e| <= sddmm_cases.sddmm_bound(S_e, D): the fp32 dot product in any order. W is invariant
    under a common shift of a row's scores, so a score error moves W_e by the factor
    exp(scale (dp_e - sum_i W_i dp_i)): at most W_e 2 scale max |dp| to first order;
  * the second term of dW is softmax_cases.forward_bound with C = 8 + 3: the effective weight is
    t_e f_s (1 / l) with f_s = 2^((m_s - M) c) the single rescale of the entry's partial: one more
    exponential (2 u) and its product (u). The exponents (p - m_s) c and (m_s - M) c are both <= 0
    and add up to d_e log2(e), so their argument roundings stay inside the 3 |d_e| u of
    forward_bound, whatever the number of segments: nothing is rescaled twice;
  * (min(n, 8 sqrt n) + 2) u sum W |V|: the n-term sum of FMAs (deterministic or Higham-Mary with
    lambda = 8), the lane groups' and partials' additions being part of those n - 1 additions, plus
    the product with f_s and the final product with 1 / l.
lse_bound: |LSE - ref| <= scale max |dp| + (3 sum W |d| + min(n, 8 sqrt n) + 5 + 2 |ln l|) u
    + (|m scale| + |LSE|) u + n 2^-125: log-sum-exp is 1-Lipschitz in the largest score error; l carries
    the relative error of its terms (3 |d| + 2 each, weighted by W), of its sum and of the rescale
    and product (3); logf is within 1 ulp (2 u |ln l|); m scale and the final sum round once each.
No constant is taken from a GPU result.

attention_emulate restates the documented summation order in numpy fp32 over the library's own
host lists (bsmr.spmm_lists at side 1 and the exported chunk), with the mutations
test_attention_ref_cpu.py uses to show that the checks reject a subtly wrong kernel.
"""
import functools

import numpy as np

import bsmr
import softmax_cases as SC
import spmm_cases
from bsmr import BF16, F16, F32
from sddmm_cases import as_seen, sddmm_bound, signed_data
from softmax_cases import FILL_BITS, _butterfly, filled, make_plan  # noqa: F401

U = 2.0 ** -24
C_ATTN = SC.C_FWD + 3.0
LOG2E = SC.LOG2E
DTYPE_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
SCALES_EXACT = [1.0, 0.125]


def limits():
    """dict(chunk, max_row_bytes): the library's constants, never a copied number."""
    return bsmr.attention_limits()


def _rows_of(lens):
    lens = np.asarray(lens, np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    ci = np.concatenate([np.arange(n, dtype=np.uint32) for n in lens])
    return len(lens), int(lens.max()), rp, ci


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(M, N, rowptr, colidx); callers do not modify the arrays. `long4`: one row of 4 chunk + 3
    entries and rows on both sides of one and two chunks (chunk - 1, chunk, chunk + 1, 2 chunk,
    2 chunk + 1, whatever the library's chunk) among rows of 0 - 3."""
    if name == "long4":
        c = limits()["chunk"]
        return _rows_of([2, 0, 4 * c + 3, 1, c + 1, 3, c - 1, 0, c, 2 * c, 2, 2 * c + 1])
    return SC.pattern(name)


PATTERNS = ["staircase", "hub", "zipf_shuffled", "empty", "long4"]
# fp32 and fp16 / bf16 (D, Dv): the generic and every compile-time lane form, D != Dv both ways,
# both row-byte extremes (64 and 1024 bytes)
SHAPES_F32 = [(16, 16), (32, 48), (64, 64), (48, 128), (256, 256)]
SHAPES_HALF = [(64, 64), (32, 128), (512, 512)]


def row_lengths(pat):
    return np.diff(np.asarray(pat[2], np.int64))


def entry_rows(pat):
    return spmm_cases.entry_rows(pat[0], pat[2])


def lane_form(D, Dv, dtype):
    """(L, EPL, live K lanes, live V lanes) of a launch: L = max(D, Dv) sizeof(T) / 16 lanes
    rounded up to a power of two (at least 4), EPL values per lane."""
    esz = 4 if dtype == F32 else 2
    rb = max(D, Dv) * esz
    L = 4
    while L * 16 < rb:
        L *= 2
    return L, 16 // esz, D * esz // 16, Dv * esz // 16


# ---------------------------------------------------------------- reference and bounds ----
def _row_sums(M, rp, cols, w, X):
    """float64 (M, X.shape[1]): per row the sum over its entries of w_e X[col_e, :]; column blocks
    bound the temporaries."""
    rp = np.asarray(rp, np.int64)
    live = np.nonzero(np.diff(rp))[0]
    out = np.zeros((M, X.shape[1]))
    for k0 in range(0, X.shape[1], 128):
        if len(live):
            out[live, k0:k0 + 128] = np.add.reduceat(w[:, None] * X[cols, k0:k0 + 128], rp[live], axis=0)
    return out


def attention_ref(pat, Q, K, V, scale, dtype=F32):
    """float64 dict(O, LSE, W, p, S, m, l, d, sd, n, rows) on Q, K, V rounded to `dtype` first, with
    the library's conventions: an empty row O = 0 and LSE = -inf."""
    M, N, rp, ci = pat
    Q, K, V = (as_seen(X, dtype).astype(np.float64) for X in (Q, K, V))
    rows, cols = entry_rows(pat), np.asarray(ci, np.int64)
    nnz = len(cols)
    p, S = np.empty(nnz), np.empty(nnz)
    step = max(1, (2 << 20) // Q.shape[1])
    for e0 in range(0, nnz, step):
        t = Q[rows[e0:e0 + step]] * K[cols[e0:e0 + step]]
        p[e0:e0 + step] = t.sum(axis=1)
        S[e0:e0 + step] = np.abs(t).sum(axis=1)
    sm = SC.softmax_ref(pat, p, scale)
    W = sm["W"]
    lens = row_lengths(pat)
    live = np.nonzero(lens)[0]
    starts = np.asarray(rp, np.int64)[live]
    m = np.full(M, -np.inf)
    l = np.zeros(M)
    O = np.zeros((M, V.shape[1]))
    if len(live):
        m[live] = np.maximum.reduceat(p, starts)
        l[live] = np.add.reduceat(np.exp((p - m[rows]) * float(scale)), starts)
        O = _row_sums(M, rp, cols, W, V)
    with np.errstate(divide="ignore"):
        LSE = m * float(scale) + np.log(l)
    return dict(O=O, LSE=LSE, W=W, p=p, S=S, m=m, l=l, d=sm["d"], sd=sm["sd"], n=sm["n"], rows=rows, cols=cols,
                lens=lens, scale=float(scale), V=V, D=Q.shape[1], rp=rp)


def _row_max(ref, x):
    out = np.zeros(len(ref["lens"]))
    np.maximum.at(out, ref["rows"], x)
    return out


def weight_bound(ref, C, opscale=1.0):
    """dW per entry (module docstring) with the softmax constant C."""
    dp = sddmm_bound(ref["S"], ref["D"], opscale)
    dpmax = _row_max(ref, dp)[ref["rows"]]
    W, n = ref["W"], ref["n"]
    return (W * 2.0 * ref["scale"] * dpmax +
            W * (C + 3 * ref["d"] + 3 * ref["sd"] + np.minimum(n, 8 * np.sqrt(n))) * U + 2.0 ** -125)


def _weighted(ref, w):
    """sum_e w_e |V_ek| per row and column."""
    return _row_sums(len(ref["lens"]), ref["rp"], ref["cols"], w, np.abs(ref["V"]))


def attention_bound(ref, opscale=1.0):
    """Per element of O (module docstring). opscale: the product of the operand scalings of Q and K
    (sddmm_bound's absolute term)."""
    n = ref["lens"].astype(np.float64)[:, None]
    return (_weighted(ref, weight_bound(ref, C_ATTN, opscale)) +
            (np.minimum(n, 8 * np.sqrt(n)) + 2) * U * _weighted(ref, ref["W"]))


def composed_bound(ref, opscale=1.0):
    """The same element through bsmr_sddmm, bsmr_softmax and bsmr_spmm, from their own tests'
    bounds: dW with softmax_cases' C, then spmm_cases.signed_bound_tight on sum W |V|."""
    return (_weighted(ref, weight_bound(ref, SC.C_FWD, opscale)) +
            spmm_cases.signed_bound_tight(_weighted(ref, ref["W"]), ref["lens"]))


def lse_bound(ref, opscale=1.0):
    n = ref["lens"].astype(np.float64)
    dpmax = _row_max(ref, sddmm_bound(ref["S"], ref["D"], opscale))
    sd = np.zeros(len(n))
    sd[ref["rows"]] = ref["sd"]
    with np.errstate(divide="ignore", invalid="ignore"):
        lnl = np.where(ref["l"] > 0, np.abs(np.log(ref["l"])), 0.0)
        ms = np.where(n > 0, np.abs(ref["m"] * ref["scale"]), 0.0)
        top = np.where(n > 0, np.abs(ref["LSE"]), 0.0)
    return (ref["scale"] * dpmax + (3 * sd + np.minimum(n, 8 * np.sqrt(n)) + 5 + 2 * lnl) * U + (ms + top) * U +
            n * 2.0 ** -125)


def _ratio(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.where(np.isfinite(r), r, np.inf).max()) if r.size else 0.0


def bound_ratios(O, LSE, ref, opscale=1.0):
    """(worst |O - ref| / attention_bound, worst |LSE - ref| / lse_bound); empty rows must be
    exactly 0 and -inf (ratio inf otherwise)."""
    O, LSE = np.asarray(O, np.float64), np.asarray(LSE, np.float64)
    empty = ref["lens"] == 0
    ro = _ratio(np.abs(O - ref["O"]), attention_bound(ref, opscale))
    live = ~empty
    rl = _ratio(np.abs(LSE[live] - ref["LSE"][live]), lse_bound(ref, opscale)[live])
    if empty.any() and not ((O[empty] == 0).all() and (LSE[empty] == -np.inf).all()):
        ro = rl = np.inf
    return ro, rl


def check_bound(O, LSE, ref, what, opscale=1.0):
    """O and LSE inside their bounds; prints "RATIO attention ..."; returns the two worst ratios."""
    ro, rl = bound_ratios(O, LSE, ref, opscale)
    print(f"RATIO attention O {ro:.4f} LSE {rl:.4f} {what}")
    assert ro <= 1.0, f"{what}: worst |O - ref| / bound = {ro:.3f}"
    assert rl <= 1.0, f"{what}: worst |LSE - ref| / bound = {rl:.3f}"
    return ro, rl


# ------------------------------------------------------------------------------- data ----
def selector(pat, D, Dv, order, dtype=F32, seed=5):
    """(Q, K, V, winner, pi, base): winner[i] = the column j*(i) of row i's entry with the largest
    pi (-1 for an empty row); the winning score is base (pi[winner] + 1). order: "random",
    "ascending", "descending". fp32: base = 1000, Q[:, 0] = 1 and K[j, 0] = 1000 (pi(j) + 1). fp16 and
    bf16 cannot hold that number, so there base = 1024 and the score is two exact products summed
    exactly in fp32: Q[:, 0] = Q[:, 1] = 1024, K[j, 0] = 256 a and K[j, 1] = b with pi(j) + 1 =
    256 a + b, a and b below 256 (N < 16384)."""
    M, N, rp, ci = pat
    rng = np.random.default_rng(seed)
    pi = {"random": rng.permutation(N), "ascending": np.arange(N), "descending": np.arange(N)[::-1]}[order]
    Q = np.zeros((M, D), np.float32)
    K = signed_data(N * D, seed + 1).reshape(N, D).copy()
    if dtype == F32:
        base = 1000.0
        assert N * base < 2 ** 24
        Q[:, 0] = 1.0
        K[:, 0] = base * (pi + 1.0)
    else:
        base = 1024.0
        assert N * base < 2 ** 24 and N < 256 * 256 - 1
        Q[:, :2] = base
        K[:, 0] = 256.0 * ((pi + 1) // 256)
        K[:, 1] = (pi + 1) % 256
    V = signed_data(N * Dv, seed + 2).reshape(N, Dv)
    lens = row_lengths(pat)
    winner = np.full(M, -1, np.int64)
    live = np.nonzero(lens)[0]
    if len(live):
        best = np.maximum.reduceat(pi[np.asarray(ci, np.int64)].astype(np.int64), np.asarray(rp, np.int64)[live])
        inv = np.empty(N, np.int64)
        inv[pi] = np.arange(N)
        winner[live] = inv[best]
    return Q, K, V, winner, pi, base


def selector_expected(V, winner, pi, base, scale, dtype=F32):
    """(O, LSE) the selector data must give bit for bit (fp32)."""
    Vs = as_seen(V, dtype)
    O = np.where((winner >= 0)[:, None], Vs[np.maximum(winner, 0)], np.float32(0)).astype(np.float32)
    LSE = np.where(winner >= 0, scale * base * (pi[np.maximum(winner, 0)] + 1.0), -np.inf)
    assert (LSE.astype(np.float32).astype(np.float64) == LSE).all()
    return O, LSE.astype(np.float32)


def check_exact(got, want, what):
    got, want = np.asarray(got), np.asarray(want, np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(axis=1))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} rows differ bit for bit, first {bad[:5]}: got "
                           f"{got[bad[0]].ravel()[:4]} want {want[bad[0]].ravel()[:4]}")


def signed_inputs(pat, D, Dv, kind, scale, seed=11):
    """(Q, K, V, opscale): uniform [-1, 1) operands, Q scaled by opscale so that the largest
    |p scale| is about 1 (narrow) or 8 (wide): a row's dot product has deviation sqrt(D) / 3 and the
    largest of some 10^4 of them is near 4.2 deviations."""
    M, N = pat[0], pat[1]
    opscale = np.float32({"narrow": 1.0, "wide": 8.0}[kind] / (scale * 1.4 * np.sqrt(D)))
    Q = signed_data(M * D, seed).reshape(M, D) * opscale
    K = signed_data(N * D, seed + 1).reshape(N, D)
    V = signed_data(N * Dv, seed + 2).reshape(N, Dv)
    return Q, K, V, float(opscale)


# --------------------------------------------------------------------------- emulation ----
MUTATIONS = ("drop_last_entry_of_segment", "drop_last_partial", "max_without_last_segment", "partial_not_rescaled",
             "neighbour_v_row")


def _exp2(x):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.exp2(np.asarray(x, np.float32)).astype(np.float32)


def _fma(a, b, c):
    """fp32 a b + c with one rounding (a float64 product of fp32 factors is exact)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b + c).astype(np.float32)


def _scores(Q, K, rows, cols, L, EPL, liveK):
    """p per entry as a lane group computes it: lane l one FMA per element of its chunk in element
    order, lanes past the row 0, then the xor butterfly of offsets L / 2 .. 1."""
    out = np.empty(len(rows), np.float32)
    step = max(1, (1 << 20) // Q.shape[1])
    for e0 in range(0, len(rows), step):
        q = Q[rows[e0:e0 + step]].reshape(-1, liveK, EPL)
        k = K[cols[e0:e0 + step]].reshape(-1, liveK, EPL)
        d = np.zeros((len(q), L), np.float32)
        for i in range(EPL):
            d[:, :liveK] = _fma(q[:, :, i], k[:, :, i], d[:, :liveK])
        with np.errstate(invalid="ignore", over="ignore"):
            out[e0:e0 + step] = _butterfly(d, L)[:, 0]
    return out


def attention_emulate(pat, Q, K, V, scale, dtype=F32, mutation=None):
    """(O, LSE) in fp32 as k_attention / k_attention_reduce compute them, in
    numpy over bsmr.spmm_lists(side = 1, chunk = limits()["chunk"]): per segment the scores
    (_scores), their maximum m, t = 2^((p - m) c) with c = scale log2(e) rounded once from double;
    lane group g of G = 64 / L adds the t of entries g, g + G, ... in entry order and takes one FMA
    per column; the groups are added in group order. A row of one segment gives acc (1 / l) and
    m scale + ln l; a split row takes M = max m_s, scales every partial once by 2^((m_s - M) c)
    (a rounded product) and adds l and acc in segment order. numpy's exp2 and log stand in for
    v_exp_f32 and logf, so the GPU is not expected to match this bit for bit on general data, only
    where every step is exact. mutation (MUTATIONS), a wrong kernel for test_attention_ref_cpu.py:
    "drop_last_entry_of_segment"; "drop_last_partial": the reduce leaves out a split row's last
    partial; "max_without_last_segment": M skips the last partial; "partial_not_rescaled": f_s = 1;
    "neighbour_v_row": a segment's last entry gathers the V row of the next CSR entry."""
    assert mutation is None or mutation in MUTATIONS, mutation
    M, N, rp, ci = pat
    Q, K, V = (as_seen(X, dtype) for X in (Q, K, V))
    D, Dv = Q.shape[1], V.shape[1]
    L, EPL, liveK, _ = lane_form(D, Dv, dtype)
    G = 64 // L
    sc = np.float32(scale)
    c = np.float32(np.float64(sc) * LOG2E)
    segs, src, _ = bsmr.spmm_lists(M, N, rp, ci, 1, limits()["chunk"])
    dst, first, count, part = (segs[:, i].astype(np.int64) for i in range(4))
    nS = len(segs)
    cols = src.astype(np.int64)
    assert (cols == np.asarray(ci, np.int64)).all()  # side 1: src is colidx, vpos the identity
    p = _scores(Q, K, entry_rows(pat), cols, L, EPL, liveK)
    vcols = cols.copy()
    last = first + count - 1
    if mutation == "neighbour_v_row":
        s = np.nonzero(count > 0)[0]
        vcols[last[s]] = cols[(last[s] + 1) % len(cols)]
    if mutation == "drop_last_entry_of_segment":
        count = np.maximum(count - 1, 0)
    NINF = np.float32(-np.inf)
    m = np.full(nS, NINF, np.float32)
    live = np.nonzero(count)[0]
    if len(live):
        # (segments are consecutive CSR ranges; a dropped last entry leaves gaps, so reduce per segment)
        idx = np.repeat(first[live], count[live]) + (np.arange(count[live].sum()) -
                                                     np.repeat(np.cumsum(count[live]) - count[live], count[live]))
        m[live] = np.fmax.reduceat(p[idx], np.cumsum(count[live]) - count[live])
    shift = np.where(m == NINF, np.float32(0), m).astype(np.float32)
    ls = np.zeros((nS, G), np.float32)
    acc = np.zeros((nS, G, Dv), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(-(-int(count.max(initial=0)) // G)):
            for g in range(G):
                s = np.nonzero(count > t * G + g)[0]
                if len(s) == 0:
                    break
                e = first[s] + t * G + g
                te = _exp2(((p[e] - shift[s]).astype(np.float32) * c).astype(np.float32))
                ls[s, g] = (ls[s, g] + te).astype(np.float32)
                acc[s, g] = _fma(te[:, None], V[vcols[e]], acc[s, g])
        l_seg, a_seg = ls[:, 0].copy(), acc[:, 0].copy()
        for g in range(1, G):
            l_seg = (l_seg + ls[:, g]).astype(np.float32)
            a_seg = (a_seg + acc[:, g]).astype(np.float32)

        O = np.full((M, Dv), np.nan, np.float32)
        LSE = np.full(M, np.nan, np.float32)

        def finish(rows_, mm, ll, aa):
            inv = np.where(ll == 0, np.float32(0), np.float32(1) / np.where(ll == 0, np.float32(1), ll)).astype(np.float32)
            O[rows_] = (aa * inv[:, None]).astype(np.float32)
            with np.errstate(divide="ignore"):
                LSE[rows_] = ((mm * sc).astype(np.float32) + np.log(ll).astype(np.float32)).astype(np.float32)

        direct = part == bsmr.SPMM_DIRECT
        finish(dst[direct], m[direct], l_seg[direct], a_seg[direct])
        for r in np.unique(dst[~direct]):
            s = np.nonzero(dst == r)[0]  # consecutive partial slots, in segment order
            assert (np.diff(part[s]) == 1).all()
            if mutation == "drop_last_partial":
                s = s[:-1]
            mx = np.fmax.reduce(m[s[:-1]] if mutation == "max_without_last_segment" else m[s])
            sh = np.float32(0) if mx == NINF else mx
            f = _exp2(((m[s] - sh).astype(np.float32) * c).astype(np.float32))
            if mutation == "partial_not_rescaled":
                f = np.ones(len(s), np.float32)
            fl = (f * l_seg[s]).astype(np.float32)
            fa = (f[:, None] * a_seg[s]).astype(np.float32)
            ll, aa = fl[0], fa[0]
            for i in range(1, len(s)):
                ll = np.float32(ll + fl[i])
                aa = (aa + fa[i]).astype(np.float32)
            finish(np.array([r]), np.array([mx], np.float32), np.array([ll], np.float32), aa[None, :])
    return O, LSE


# ------------------------------------------------------- device helpers (GPU tests only) ----
def attention_once(plan, Q, K, V, scale, dtype=F32, lse=True, dev=None):
    """(O, LSE) (numpy fp32; LSE None without `lse`) of one bsmr_attention on host operands. Both
    outputs start as FILL_BITS with a guard zone behind them: the launch must write every element
    and nothing behind the last. dev: (dQ, dK, dV) already on the device."""
    from gpu_util import to_device, torch_cuda
    torch = torch_cuda()
    D, Dv = Q.shape[1], V.shape[1]
    dQ, dK, dV = dev or (to_device(Q, dtype), to_device(K, dtype), to_device(V, dtype))
    bufO, dO = filled(plan.M * Dv)
    bufL, dL = filled(plan.M)
    plan.attention(dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D, Dv, dO.data_ptr(), dL.data_ptr() if lse else 0,
                   scale, stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    hO, hL = bufO.cpu().numpy(), bufL.cpu().numpy()
    assert (hO[plan.M * Dv:].view(np.uint32) == FILL_BITS).all(), "a store past the end of O"
    assert (hL[plan.M:].view(np.uint32) == FILL_BITS).all(), "a store past the end of LSE"
    O = hO[:plan.M * Dv].reshape(plan.M, Dv)
    assert not (O.view(np.uint32) == FILL_BITS).any(), "an element of O was never written"
    if not lse:
        assert (hL.view(np.uint32) == FILL_BITS).all(), "LSE written though none was asked for"
        return O, None
    assert not (hL[:plan.M].view(np.uint32) == FILL_BITS).any(), "an element of LSE was never written"
    return O, hL[:plan.M]
