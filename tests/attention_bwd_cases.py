"""Patterns, float64 reference, data sets, bounds and a numpy-fp32 emulation of the fused sparse
attention backward (bsmr_attention_backward). No GPU here:
tests/test_attention_bwd_ref_cpu.py checks this module; test_gpu_attention_bwd_float64.py,
test_gpu_attention_bwd_edges.py, test_gpu_attention_bwd_autograd.py and test_gpu_far_attention_bwd.py
use it. It builds on attention_cases, spmm_cases and softmax_cases and reads every constant from
bsmr.attention_backward_limits().

Reference: backward_ref, the definition in numpy float64 on Q, K, V rounded to the dtype and the
given fp32 O, GO and LSE; the kernel is a function of those six inputs, whoever produced O and LSE:
    p = dot(Q_i, K_j), x = p scale, w = LSE_i == -inf ? 0 : exp(x - LSE_i) (0 under 2^-126, as
    v_exp_f32 gives it), g = dot(GO_i, V_j),
    delta_i = dot(GO_i, O_i), dp = w (g - delta_i) scale,
    GQ_i = sum_e dp K_j, GK_j = sum_{e in column j} dp Q_i, GV_j = sum w GO_i.

Patterns: attention_cases.PATTERNS and the transpose of each ("<name>_T"), so that the columns also
see every list length 0 .. 271, the 2048 hub, empty columns and, for long4, chunk - 1 .. 4 chunk + 3
around the library's col_chunk (long4 itself is built around row_chunk).

Exact data (a right kernel equals float64 bit for bit in any summation order):
  * selector: attention_cases.selector with LSE and O what the forward gives exactly (scale base
    (pi(j*) + 1) and V[j*]) and GO on the k/8 grid. The winner's x equals LSE bit for bit, so its
    w = 2^0 = 1; every other x lies at least 125 below and its w underflows to 0. g and delta of a
    winner are the same dot product in the same order, so dp = +-0 and GQ = GK = 0, and
    GV[j] = sum of GO[i] over the rows that j wins: at most 2^12 grid values, exact in any order;
  * flat: Q non-zero in the first half of its columns only and K in the second (both k/8), so every
    p is exactly 0; LSE = 0, so every w is exactly 1; GO[i] = +-e_c(i); V and O on the k/8 grid.
    g and delta are single grid values, |g - delta| <= 8, a multiple of 1/8; a term of GQ / GK is at
    most 8 * 4 = 2^11 units of 1/64 (times the power-of-two scale), and a list of up to 2^13 of them
    sums exactly in fp32 in any order. Every entry contributes to GQ, GK and GV.

Bound (signed data), per element, u = 2^-24, n the destination's list length, first order in u:
    ep = sddmm_bound(S_p, D), eg = sddmm_bound(S_g, Dv), ed = sddmm_bound(S_delta, Dv)     (section 11.1)
    dw = w (scale ep + (C1 + C2 (|x| + |LSE|) + C3 |x - LSE|) u) + 2^-125
    ddp = scale (dw |g - delta| + w (eg + ed) + 3 u w |g - delta|)
    |GQ - ref| <= sum_e ddp |K| + min(n, 8 sqrt n) u sum_e |dp K|
    |GK - ref| <= sum_e ddp |Q| + min(n, 8 sqrt n) u sum_e |dp Q|
    |GV - ref| <= sum_e dw |GO| + min(n, 8 sqrt n) u sum_e w |GO|
  counted from weight_of's operation sequence (csrc/attention_bwd.hip):
    x = p scale            one rounding, |x| u in the exponent:           C2 = 1 (on |x| alone; |LSE|
                           is carried for the form's sake and only loosens the bound)
    d = x - LSE            one rounding, |d| u
    t = d log2e_f32        one rounding and the constant's own error (< 2^-25 relative), 2 |d| u:
                                                                          C3 = 1 + 2 = 3
    w = v_exp_f32(t)       documented at 1 ulp = 2 u:                     C1 = 2
  The |x - LSE| term is new against section 13: the shift is by LSE, not by the segment's maximum,
  so x - LSE is not an exact difference of nearby numbers and is not <= 0 by construction.
  2^-125: v_exp_f32 flushes results under 2^-126. In ddp: g - delta rounds once (u |g - delta|) and
  carries both dot-product errors; the products with w and with scale round once each (3 u together
  with the difference). The n-term FMA sums use min(n, 8 sqrt n) u sum |terms| as section 13 does
  (deterministic or Higham-Mary with lambda = 8), the lane groups' and partials' additions being
  part of those n - 1 additions. No constant is taken from a GPU result.

backward_emulate restates the documented order in numpy fp32 over bsmr.spmm_lists (side 1 at
row_chunk, side 2 at col_chunk), with the mutations test_attention_bwd_ref_cpu.py uses to show that
the checks reject a subtly wrong kernel.
"""
import functools

import numpy as np

import attention_cases as AC
import bsmr
import softmax_cases as SC
import spmm_cases
from attention_cases import DTYPE_NAME, SCALES_EXACT, SHAPES_F32, SHAPES_HALF, check_exact, lane_form  # noqa: F401
from bsmr import BF16, F16, F32  # noqa: F401
from sddmm_cases import as_seen, grid_data, sddmm_bound, signed_data
from softmax_cases import FILL_BITS, filled, make_plan  # noqa: F401

U = 2.0 ** -24
C1, C2, C3 = 2.0, 1.0, 3.0
LOG2E = 1.4426950408889634
LOG2E_F32 = np.float32(LOG2E)
OUTPUTS = ("GQ", "GK", "GV")


def limits():
    """dict(row_chunk, col_chunk, max_row_bytes): the library's constants, never a copied number."""
    return bsmr.attention_backward_limits()


def transpose(pat):
    """The pattern of S^T: row j holds the rows of column j in ascending order."""
    M, N, rp, ci = pat
    rows = spmm_cases.entry_rows(M, rp)
    order = np.argsort(np.asarray(ci, np.int64), kind="stable")
    rpt = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=N))]).astype(np.uint32)
    return N, M, rpt, rows[order].astype(np.uint32)


def _long4(chunk):
    c = chunk
    return AC._rows_of([2, 0, 4 * c + 3, 1, c + 1, 3, c - 1, 0, c, 2 * c, 2, 2 * c + 1])


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(M, N, rowptr, colidx) of an attention_cases pattern or, "<name>_T", its transpose. long4 has
    its row lengths around row_chunk, long4_T its column lengths around col_chunk."""
    if name == "long4":
        return _long4(limits()["row_chunk"])
    if name == "long4_T":
        return transpose(_long4(limits()["col_chunk"]))
    if name.endswith("_T"):
        return transpose(AC.pattern(name[:-2]))
    return AC.pattern(name)


PATTERNS = AC.PATTERNS + [n + "_T" for n in AC.PATTERNS]


def col_lengths(pat):
    return np.bincount(pat[3], minlength=pat[1]).astype(np.int64)


def expected_stats(pat, D=0, Dv=0, built=True):
    """Plan.attention_backward_stats() as the list lengths give it, by spmm_cases.expected_stats;
    the scratch sizes for a plan that has only ever been prepared or launched at (D, Dv)."""
    lim = limits()
    out = dict(row_segments=0, row_split=0, row_partials=0, row_max=0, row_chunk=lim["row_chunk"], col_segments=0,
               col_split=0, col_partials=0, col_max=0, col_chunk=lim["col_chunk"], row_scratch_bytes=0,
               col_scratch_bytes=0, delta_bytes=0)
    if not built:
        return out
    for side, name in ((1, "row"), (2, "col")):
        e = spmm_cases.expected_stats(pat, side, lim[name + "_chunk"])
        out.update({f"{name}_segments": e["segments"], f"{name}_split": e["split_dsts"],
                    f"{name}_partials": e["partials"], f"{name}_max": e["max_list"]})
    out["row_scratch_bytes"] = 4 * out["row_partials"] * D
    out["col_scratch_bytes"] = 4 * out["col_partials"] * (D + Dv)
    out["delta_bytes"] = 4 * pat[0]
    return out


# ---------------------------------------------------------------- reference and bounds ----
def _dst_sums(n, dst, w, X, src):
    """float64 (n, X.shape[1]): per destination the sum over its entries of w_e X[src_e, :]."""
    out = np.zeros((n, X.shape[1]))
    if len(dst) == 0:
        return out
    order = np.argsort(dst, kind="stable")
    cnt = np.bincount(dst, minlength=n)
    live = np.nonzero(cnt)[0]
    starts = (np.cumsum(cnt) - cnt)[live]
    for k0 in range(0, X.shape[1], 128):
        out[live, k0:k0 + 128] = np.add.reduceat(w[order, None] * X[src[order], k0:k0 + 128], starts, axis=0)
    return out


def _dots(A, B, ia, ib):
    """(sum_k a b, sum_k |a b|) per pair, float64, in blocks."""
    n = len(ia)
    p, S = np.empty(n), np.empty(n)
    step = max(1, (2 << 20) // A.shape[1])
    for e0 in range(0, n, step):
        t = A[ia[e0:e0 + step]] * B[ib[e0:e0 + step]]
        p[e0:e0 + step] = t.sum(axis=1)
        S[e0:e0 + step] = np.abs(t).sum(axis=1)
    return p, S


def backward_ref(pat, Q, K, V, O, GO, LSE, scale, dtype=F32, keep64=False):
    """float64 dict(GQ, GK, GV, ...) of the definition on Q, K, V rounded to `dtype` and the given
    fp32 O, GO, LSE (keep64: taken as the float64 values they are), with what the bounds need."""
    M, N, rp, ci = pat
    with np.errstate(invalid="ignore", over="ignore"):
        Q, K, V = (as_seen(X, dtype).astype(np.float64) for X in (Q, K, V))
        O, GO, LSE = (np.asarray(X, np.float64 if keep64 else np.float32).astype(np.float64) for X in (O, GO, LSE))
        rows, cols = spmm_cases.entry_rows(M, rp), np.asarray(ci, np.int64)
        p, Sp = _dots(Q, K, rows, cols)
        g, Sg = _dots(GO, V, rows, cols)
        every = np.arange(M)
        delta, Sd = _dots(GO, O, every, every)
        x = p * float(scale)
        lse = LSE[rows]
        d = x - np.where(lse == -np.inf, 0.0, lse)
        # v_exp_f32 gives 0 under 2^-126, and so does the definition (the bound's 2^-125 covers the edge)
        w = np.where((lse == -np.inf) | (d * LOG2E < -126.0), 0.0, np.exp(d))
        gd = g - delta[rows]
        dp = w * gd * float(scale)
    return dict(GQ=_dst_sums(M, rows, dp, K, cols), GK=_dst_sums(N, cols, dp, Q, rows),
                GV=_dst_sums(N, cols, w, GO, rows), p=p, Sp=Sp, g=g, Sg=Sg, delta=delta, Sd=Sd, x=x, w=w, gd=gd, dp=dp,
                lse=lse, rows=rows, cols=cols, Q=Q, K=K, V=V, GO=GO, scale=float(scale), M=M, N=N, D=Q.shape[1],
                Dv=V.shape[1], rlen=AC.row_lengths(pat), clen=col_lengths(pat))


def _sum_term(n):
    n = np.asarray(n, np.float64)[:, None]
    return np.minimum(n, 8 * np.sqrt(n)) * U


def entry_bounds(ref, opscale=1.0):
    """(dw, ddp) per entry (module docstring). opscale: the product of the operand scalings of Q
    and K (sddmm_bound's absolute term)."""
    with np.errstate(invalid="ignore"):
        ep = sddmm_bound(ref["Sp"], ref["D"], opscale)
        eg = sddmm_bound(ref["Sg"], ref["Dv"])
        ed = sddmm_bound(ref["Sd"], ref["Dv"])[ref["rows"]]
        lse = np.where(np.isfinite(ref["lse"]), ref["lse"], 0.0)
        x, w, s = ref["x"], ref["w"], ref["scale"]
        dw = w * (s * ep + (C1 + C2 * (np.abs(x) + np.abs(lse)) + C3 * np.abs(x - lse)) * U) + 2.0 ** -125
        agd = np.abs(ref["gd"])
        ddp = s * (dw * agd + w * (eg + ed) + 3 * U * w * agd)
    return dw, ddp


def backward_bound(ref, opscale=1.0):
    """dict(GQ, GK, GV) of per-element bounds (module docstring)."""
    dw, ddp = entry_bounds(ref, opscale)
    rows, cols, M, N = ref["rows"], ref["cols"], ref["M"], ref["N"]
    aK, aQ, aGO = np.abs(ref["K"]), np.abs(ref["Q"]), np.abs(ref["GO"])
    adp = np.abs(ref["dp"])
    return dict(GQ=_dst_sums(M, rows, ddp, aK, cols) + _sum_term(ref["rlen"]) * _dst_sums(M, rows, adp, aK, cols),
                GK=_dst_sums(N, cols, ddp, aQ, rows) + _sum_term(ref["clen"]) * _dst_sums(N, cols, adp, aQ, rows),
                GV=_dst_sums(N, cols, dw, aGO, rows) + _sum_term(ref["clen"]) * _dst_sums(N, cols, ref["w"], aGO, rows))


def composed_bound(ref, fwd, opscale=1.0):
    """The same three gradients through attention's backward launches (bsmr_sddmm, bsmr_softmax,
    bsmr_sddmm, bsmr_spmm_t, bsmr_softmax_backward, bsmr_spmm, bsmr_spmm_t), from their own tests'
    bounds, against backward_ref. fwd: attention_cases.attention_ref of the same operands, whose W
    is the reference's w up to the rounding of the given LSE and O to fp32 (relative |LSE| u in w, u
    S_delta in delta), which is added.
      dW: attention_cases.weight_bound with softmax_cases' C;  dg: sddmm_bound (fp32 SDDMM of GO and V);
      dP = scale W (g - r), r = sum_i W g: softmax_cases.backward_bound on exact inputs plus the
      propagation scale (dW |g - r| + W (dg + sum_i (dW_i |g_i| + W_i dg_i)));
      the three SpMM: spmm_cases.signed_bound_tight on sum |terms| plus sum (value error) |operand|."""
    rows, cols, M, N = ref["rows"], ref["cols"], ref["M"], ref["N"]
    s = ref["scale"]
    W, g = fwd["W"], ref["g"]
    lse = np.where(np.isfinite(ref["lse"]), ref["lse"], 0.0)
    dW = AC.weight_bound(fwd, SC.C_FWD, opscale) + W * np.abs(lse) * U
    dg = sddmm_bound(ref["Sg"], ref["Dv"])
    sref = SC.backward_ref((M, N, fwd["rp"], None), W, g, s)
    r = sref["r"]
    pat_rows = (M, N, fwd["rp"], None)
    prop = SC._per_row(pat_rows, dW * np.abs(g) + W * dg, np.add)[rows] + U * ref["Sd"][rows]
    dgp = SC.backward_bound(sref) + s * (dW * np.abs(g - r) + W * (dg + prop))
    agp = np.abs(sref["dP"])
    aK, aQ, aGO = np.abs(ref["K"]), np.abs(ref["Q"]), np.abs(ref["GO"])
    tight = spmm_cases.signed_bound_tight
    return dict(GQ=_dst_sums(M, rows, dgp, aK, cols) + tight(_dst_sums(M, rows, agp, aK, cols), ref["rlen"], opscale),
                GK=_dst_sums(N, cols, dgp, aQ, rows) + tight(_dst_sums(N, cols, agp, aQ, rows), ref["clen"], opscale),
                GV=_dst_sums(N, cols, dW, aGO, rows) + tight(_dst_sums(N, cols, W, aGO, rows), ref["clen"]))


def bound_ratios(got, ref, opscale=1.0):
    """dict(GQ, GK, GV) of worst |got - ref| / bound; destinations without entries must be exactly 0
    (ratio inf otherwise)."""
    bound = backward_bound(ref, opscale)
    out = {}
    for name, lens in (("GQ", ref["rlen"]), ("GK", ref["clen"]), ("GV", ref["clen"])):
        if got.get(name) is None:
            continue
        Y = np.asarray(got[name], np.float64)
        r = AC._ratio(np.abs(Y - ref[name]), bound[name])
        if (lens == 0).any() and not (Y[lens == 0] == 0).all():
            r = np.inf
        out[name] = r
    return out


def check_bound(got, ref, what, opscale=1.0):
    """Every given gradient inside its bound; prints "RATIO attention_bwd ..."; returns the ratios."""
    r = bound_ratios(got, ref, opscale)
    print("RATIO attention_bwd " + " ".join(f"{k} {v:.4f}" for k, v in r.items()) + f" {what}")
    for k, v in r.items():
        assert v <= 1.0, f"{what}: worst |{k} - ref| / bound = {v:.3f}"
    return r


def check_exact_all(got, ref, what):
    """Every given gradient equals the float64 reference bit for bit."""
    for name in OUTPUTS:
        if got.get(name) is not None:
            want = ref[name].astype(np.float32)
            assert (want.astype(np.float64) == ref[name]).all(), f"{what}: the reference {name} is not an fp32 value"
            check_exact(got[name], want + np.float32(0), f"{name} {what}")


# ------------------------------------------------------------------------------- data ----
def selector_inputs(pat, D, Dv, order, scale, dtype=F32, seed=5):
    """(Q, K, V, O, GO, LSE, winner): attention_cases.selector with the forward's exact outputs and
    GO on the k/8 grid."""
    Q, K, V, winner, pi, base = AC.selector(pat, D, Dv, order, dtype, seed)
    O, LSE = AC.selector_expected(V, winner, pi, base, scale, dtype)
    GO = grid_data(pat[0] * Dv, seed + 3).reshape(pat[0], Dv)
    return Q, K, V, O, GO, LSE, winner


def selector_expected(pat, GO, winner, D, Dv):
    """(GQ, GK, GV) fp32 the selector data must give bit for bit: zeros, zeros, and per column the
    sum of GO over the rows it wins."""
    M, N = pat[0], pat[1]
    GV = np.zeros((N, Dv))
    np.add.at(GV, winner[winner >= 0], GO[winner >= 0].astype(np.float64))
    return np.zeros((M, D), np.float32), np.zeros((N, D), np.float32), GV.astype(np.float32)


def flat_inputs(pat, D, Dv, dtype=F32, seed=17):
    """(Q, K, V, O, GO, LSE) of the flat set (module docstring)."""
    M, N = pat[0], pat[1]
    Q = grid_data(M * D, seed).reshape(M, D).copy()
    K = grid_data(N * D, seed + 1).reshape(N, D).copy()
    Q[:, D // 2:] = 0
    K[:, :D // 2] = 0
    V = grid_data(N * Dv, seed + 2).reshape(N, Dv)
    O = grid_data(M * Dv, seed + 3).reshape(M, Dv)
    rng = np.random.default_rng(seed + 4)
    GO = np.zeros((M, Dv), np.float32)
    GO[np.arange(M), rng.integers(0, Dv, M)] = rng.choice(np.float32([-1, 1]), M)
    return Q, K, V, O, GO, np.zeros(M, np.float32)


def signed_inputs(pat, D, Dv, kind, scale, dtype=F32, seed=11):
    """(Q, K, V, O, GO, LSE, opscale, fwd): attention_cases.signed_inputs, O and LSE from
    attention_ref rounded to fp32, GO uniform in [-1, 1); fwd is that attention_ref."""
    Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, kind, scale, seed)
    fwd = AC.attention_ref(pat, Q, K, V, scale, dtype)
    GO = signed_data(pat[0] * Dv, seed + 3).reshape(pat[0], Dv)
    return Q, K, V, fwd["O"].astype(np.float32), GO, fwd["LSE"].astype(np.float32), opscale, fwd


# --------------------------------------------------------------------------- emulation ----
MUTATIONS = ("drop_last_entry_of_col_segment", "drop_last_col_partial", "no_delta", "dp_without_scale",
             "neighbour_lse_on_cols", "gk_takes_k")


def _f32(x):
    return np.asarray(x, np.float32)


def _entry_values(Q, K, V, O, GO, LSE, rows, cols, scale, L, EPL, liveK, liveV, lse_rows=None, no_delta=False,
                  no_scale=False):
    """(w, dp) fp32 per entry as weight_of computes them from the lane-group dot products."""
    M = len(LSE)
    sc = np.float32(scale)
    p = AC._scores(Q, K, rows, cols, L, EPL, liveK)
    g = AC._scores(GO, V, rows, cols, L, EPL, liveV)
    every = np.arange(M)
    delta = AC._scores(GO, O, every, every, L, EPL, liveV) if M else np.zeros(0, np.float32)
    if no_delta:
        delta = np.zeros(M, np.float32)
    lse = LSE[rows if lse_rows is None else lse_rows]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        x = _f32(p * sc)
        t = _f32(_f32(x - lse) * LOG2E_F32)
        w = np.where(lse == -np.inf, np.float32(0), AC._exp2(t)).astype(np.float32)
        wg = _f32(w * _f32(g - delta[rows]))
        dp = wg if no_scale else _f32(wg * sc)
    return w, dp


def _accumulate(segs, coef, X, src, ndst, G, drop_last_entry=False, drop_last_partial=False, shuffle=None):
    """Y (ndst x X.shape[1]) fp32: per segment, lane group g of G takes the list entries g, g + G, ...
    in entry order, one FMA per element; the groups are added in group order, a split destination's
    partials in segment order. coef and src are per list position. shuffle: a Generator; the
    entries of every segment are taken in a random order instead (the exact sets must not care)."""
    dst, first, count, part = (segs[:, i].astype(np.int64) for i in range(4))
    nS, Kc = len(segs), X.shape[1]
    if drop_last_entry:
        count = np.maximum(count - 1, 0)
    acc = np.zeros((nS, G, Kc), np.float32)
    perm = None
    if shuffle is not None:
        perm = np.arange(len(coef))
        for s in np.nonzero(count > 1)[0]:
            shuffle.shuffle(perm[first[s]:first[s] + count[s]])
    for t in range(-(-int(count.max(initial=0)) // G)):
        for g in range(G):
            s = np.nonzero(count > t * G + g)[0]
            if len(s) == 0:
                break
            e = first[s] + t * G + g
            if perm is not None:
                e = perm[e]
            acc[s, g] = AC._fma(coef[e][:, None], X[src[e]], acc[s, g])
    with np.errstate(invalid="ignore", over="ignore"):
        a_seg = acc[:, 0].copy()
        for g in range(1, G):
            a_seg = (a_seg + acc[:, g]).astype(np.float32)
        Y = np.full((ndst, Kc), np.nan, np.float32)
        direct = part == bsmr.SPMM_DIRECT
        Y[dst[direct]] = a_seg[direct]
        for r in np.unique(dst[~direct]):
            s = np.nonzero(dst == r)[0]
            assert (np.diff(part[s]) == 1).all()
            if drop_last_partial:
                s = s[:-1]
            if shuffle is not None:
                s = shuffle.permutation(s)
            tot = a_seg[s[0]]
            for i in s[1:]:
                tot = (tot + a_seg[i]).astype(np.float32)
            Y[r] = tot
    return Y


def backward_emulate(pat, Q, K, V, O, GO, LSE, scale, dtype=F32, mutation=None, shuffle=None):
    """dict(GQ, GK, GV) in fp32 as the kernels compute them, in numpy over
    bsmr.spmm_lists. numpy's exp2 stands in for v_exp_f32, so the GPU is not expected to match this
    bit for bit on general data, only where every step is exact. mutation (MUTATIONS), a wrong kernel
    for test_attention_bwd_ref_cpu.py: "drop_last_entry_of_col_segment"; "drop_last_col_partial": the
    columns' reduce leaves out a split column's last partial; "no_delta": delta = 0;
    "dp_without_scale"; "neighbour_lse_on_cols": the column side gathers LSE of row i + 1;
    "gk_takes_k": GK accumulates K[j] where it should take Q[i]."""
    assert mutation is None or mutation in MUTATIONS, mutation
    M, N, rp, ci = pat
    Q, K, V = (as_seen(X, dtype) for X in (Q, K, V))
    O, GO, LSE = _f32(O), _f32(GO), _f32(LSE)
    D, Dv = Q.shape[1], V.shape[1]
    L, EPL, liveK, liveV = lane_form(D, Dv, dtype)
    G = 64 // L
    lim = limits()
    rows, cols = spmm_cases.entry_rows(M, rp), np.asarray(ci, np.int64)
    kw = dict(no_delta=mutation == "no_delta", no_scale=mutation == "dp_without_scale")
    w, dp = _entry_values(Q, K, V, O, GO, LSE, rows, cols, scale, L, EPL, liveK, liveV, **kw)
    rsegs, rsrc, _ = bsmr.spmm_lists(M, N, rp, ci, 1, lim["row_chunk"])
    assert (rsrc.astype(np.int64) == cols).all()
    GQ = _accumulate(rsegs, dp, K, cols, M, G, shuffle=shuffle)
    csegs, csrc, cvpos = bsmr.spmm_lists(M, N, rp, ci, 2, lim["col_chunk"])
    csrc, cvpos = csrc.astype(np.int64), cvpos.astype(np.int64)
    assert (rows[cvpos] == csrc).all()
    wc, dpc = w, dp
    if mutation == "neighbour_lse_on_cols":
        wc, dpc = _entry_values(Q, K, V, O, GO, LSE, rows, cols, scale, L, EPL, liveK, liveV, lse_rows=(rows + 1) % M)
    ckw = dict(drop_last_entry=mutation == "drop_last_entry_of_col_segment",
               drop_last_partial=mutation == "drop_last_col_partial", shuffle=shuffle)
    if mutation == "gk_takes_k":
        GK = _accumulate(csegs, dpc[cvpos], K, cols[cvpos], N, G, **ckw)
    else:
        GK = _accumulate(csegs, dpc[cvpos], Q, csrc, N, G, **ckw)
    GV = _accumulate(csegs, wc[cvpos], GO, csrc, N, G, **ckw)
    return dict(GQ=GQ, GK=GK, GV=GV)


# ------------------------------------------------------- device helpers (GPU tests only) ----
def backward_once(plan, Q, K, V, O, GO, LSE, scale, dtype=F32, want=OUTPUTS, dev=None):
    """dict(GQ, GK, GV) (numpy fp32; None for an output not in `want`) of one
    bsmr_attention_backward on host operands. Every output starts as FILL_BITS with a guard zone
    behind it: the launch must write every element of a requested output, nothing behind its last
    and nothing of one that was not requested. dev: the six operands already on the device."""
    from gpu_util import torch_cuda
    torch = torch_cuda()
    D, Dv = Q.shape[1], V.shape[1]
    d = dev or device_inputs(Q, K, V, O, GO, LSE, dtype)
    shapes = dict(GQ=(plan.M, D), GK=(plan.N, D), GV=(plan.N, Dv))
    bufs = {k: filled(r * c) for k, (r, c) in shapes.items()}
    ptr = {k: (bufs[k][1].data_ptr() if k in want else 0) for k in OUTPUTS}
    plan.attention_backward(*(t.data_ptr() for t in d), D, Dv, ptr["GQ"], ptr["GK"], ptr["GV"], scale,
                            stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    out = {}
    for k, (r, c) in shapes.items():
        h = bufs[k][0].cpu().numpy()
        if k not in want:
            assert (h.view(np.uint32) == FILL_BITS).all(), f"{k} written though it was not asked for"
            out[k] = None
            continue
        assert (h[r * c:].view(np.uint32) == FILL_BITS).all(), f"a store past the end of {k}"
        Y = h[:r * c].reshape(r, c)
        assert not (Y.view(np.uint32) == FILL_BITS).any(), f"an element of {k} was never written"
        out[k] = Y
    return out


def device_inputs(Q, K, V, O, GO, LSE, dtype=F32):
    """(dQ, dK, dV, dO, dGO, dLse): Q, K, V in `dtype`, the others fp32 (LSE of at least one element)."""
    from gpu_util import to_device
    lse = _f32(LSE) if len(LSE) else np.zeros(1, np.float32)
    return (to_device(Q, dtype), to_device(K, dtype), to_device(V, dtype), to_device(_f32(O), F32),
            to_device(_f32(GO), F32), to_device(lse, F32))


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or
               (a[k].shape == b[k].shape and bool((a[k].view(np.uint32) == b[k].view(np.uint32)).all())) for k in OUTPUTS)
