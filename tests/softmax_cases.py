"""Patterns, float64 references, data sets, bounds and a numpy-fp32 emulation of the row softmax over
the plan's pattern (bsmr_softmax / bsmr_softmax_backward). No GPU here:
tests/test_softmax_ref_cpu.py checks this module; test_softmax_items_cpu.py,
test_gpu_softmax_float64.py, test_gpu_softmax_edges.py and test_gpu_attention_autograd.py use it.

References: softmax_ref / backward_ref, numpy float64 straight from the CSR.

Forward data (P, one value per stored entry):
  * one-hot: per row one entry +2000, the others -2000. d = -4000 scale <= -500 underflows to
    exactly 0, exp(0) = 1 and 1 / 1 = 1, so W must equal the one-hot vector bit for bit; without
    the max subtraction exp(2000 scale) overflows. The hot position is (7 i) mod len, or a fixed
    place (first, last, both sides of every pass boundary);
  * grid: multiples of 1/8 in [-4, 4); adding 1000 or 4096 to a row is exact on that grid, so W of
    the shifted rows must equal the unshifted W bit for bit;
  * window: 64 consecutive entries 0, the rest -2000: W = 1/64 inside, exactly 0 outside;
  * signed: narrow [-1, 1) and wide [-8, 8), held to forward_bound.

forward_bound, per entry, with u = 2^-24, n the row length, d_e = (P_e - max) scale:
    |W - ref| <= ref (C + 3 |d_e| + 3 sum_i ref |d| + min(n, 8 sqrt n)) u + 2^-125
  3 |d_e|: the subtraction, the factor scale log2(e) rounded once from double, and their product,
  each to half an ulp, ahead of the exponential (numerator; the sum_i term is the same for the
  denominator's terms); min(n, 8 sqrt n): the n-term positive sum, deterministic or Higham-Mary
  with lambda = 8; C = 8: the exponential (v_exp_f32, documented at 1 ulp = 2 u) once for the
  numerator and once for the denominator's terms, the reciprocal (correctly rounded, u), the final
  product (u), and 2 u of slack for the rescaling of a running sum between the passes of a row
  longer than block_pass. 2^-125: v_exp_f32 flushes results under 2^-126.
Row sums are within (n + C) u of 1.

Backward data: grid (W signed powers of two in [1/4, 4], G multiples of 1/8 in [-4, 4), scale a
power of two: every product is a multiple of 2^-5 and every sum of n <= 2^15 of them fits 24 bits,
so dP is exact in any order) and signed, held to backward_bound:
    |dP - ref| <= scale |W_e| [(min(2 n, 8 sqrt n) + 2) u sum_i |W G| + 3 u (|G_e| + |r|)] + 1e-6 scale.

softmax_emulate restates the documented summation order in numpy fp32 over the library's own
host item list (bsmr.softmax_items), with the mutations test_softmax_ref_cpu.py uses to show that
the checks reject a subtly wrong kernel.
"""
import functools

import numpy as np

import bsmr
import spmm_cases
from sddmm_cases import grid_data, signed_data
from small_patterns import SMALL

U = 2.0 ** -24
C_FWD = 8.0
SCALES = [1.0, 0.125, 64 ** -0.5]
HOT, COLD = np.float32(2000.0), np.float32(-2000.0)


def limits():
    """dict(wave_max, block_pass): the library's constants, never a copied number."""
    return bsmr.softmax_limits()


def _rows_of(lens):
    lens = np.asarray(lens, np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    ci = np.concatenate([np.arange(n, dtype=np.uint32) for n in lens])
    return len(lens), int(lens.max()), rp, ci


def long_lengths():
    lim = limits()
    w, b = lim["wave_max"], lim["block_pass"]
    return [2, w, 1, w + 1, 3, b, 0, b + 1, 1, 2 * b + 37, 2]


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(M, N, rowptr, colidx); callers do not modify the arrays. `long`: rows of exactly wave_max,
    wave_max + 1, block_pass, block_pass + 1 and 2 block_pass + 37 entries among rows of 0 - 3."""
    if name == "long":
        return _rows_of(long_lengths())
    if name in SMALL:
        return SMALL[name]
    return spmm_cases.pattern(name)


PATTERNS = ["staircase", "hub", "zipf_shuffled", "empty", "long"]
SMALLEST = sorted(SMALL)


def row_lengths(pat):
    return np.diff(np.asarray(pat[2], np.int64))


def entry_rows(pat):
    return spmm_cases.entry_rows(pat[0], pat[2])


def _per_row(pat, x, op):
    """op.reduceat over the rows of x (nnz): (value per non-empty row scattered to M, with `fill`
    left out: the caller indexes by entry_rows, which never names an empty row)."""
    lens = row_lengths(pat)
    live = np.nonzero(lens)[0]
    out = np.zeros(pat[0], x.dtype)
    if len(live):
        out[live] = op.reduceat(x, np.asarray(pat[2], np.int64)[live])
    return out


# ---------------------------------------------------------------- references and bounds ----
def softmax_ref(pat, P, scale):
    """float64 dict(W, d = |d_e|, sd = sum_i W |d| per entry, n = row length per entry) with the
    library's conventions: -inf weight 0, a row of nothing but -inf zeros, NaN / +inf rows NaN."""
    rows = entry_rows(pat)
    P = np.asarray(P, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = _per_row(pat, P, np.maximum)
        m = np.where(m == -np.inf, 0.0, m)
        d = (P - m[rows]) * float(scale)
        t = np.exp(d)
        s = _per_row(pat, t, np.add)
        W = np.where(s[rows] == 0, 0.0, t / np.where(s == 0, 1.0, s)[rows])
        ad = np.where(np.isfinite(d), np.abs(d), 0.0)
        sd = _per_row(pat, np.where(np.isfinite(W), W, 0.0) * ad, np.add)[rows]
    return dict(W=W, d=ad, sd=sd, n=row_lengths(pat)[rows].astype(np.float64))


def forward_bound(ref):
    n = ref["n"]
    return ref["W"] * (C_FWD + 3 * ref["d"] + 3 * ref["sd"] + np.minimum(n, 8 * np.sqrt(n))) * U + 2.0 ** -125


def forward_ratio(W, ref, mask=None):
    """max |W - ref| / forward_bound over the entries of `mask` (inf where W is not finite)."""
    r = np.abs(np.asarray(W, np.float64) - ref["W"]) / forward_bound(ref)
    r = np.where(np.isfinite(r), r, np.inf)
    if mask is not None:
        r = r[mask]
    return float(r.max()) if r.size else 0.0


def row_sum_ratio(pat, W):
    """max over non-empty rows of |sum W - 1| / ((n + C) u)."""
    lens = row_lengths(pat)
    s = _per_row(pat, np.asarray(W, np.float64), np.add)
    live = lens > 0
    r = np.abs(s[live] - 1.0) / ((lens[live] + C_FWD) * U)
    return float(np.where(np.isfinite(r), r, np.inf).max()) if r.size else 0.0


def backward_ref(pat, W, G, scale):
    rows = entry_rows(pat)
    W, G = np.asarray(W, np.float64), np.asarray(G, np.float64)
    r = _per_row(pat, W * G, np.add)[rows]
    sa = _per_row(pat, np.abs(W * G), np.add)[rows]
    return dict(dP=float(scale) * W * (G - r), W=W, G=G, r=r, sa=sa, n=row_lengths(pat)[rows].astype(np.float64),
                scale=float(scale))


def backward_bound(ref):
    n = ref["n"]
    return ref["scale"] * np.abs(ref["W"]) * ((np.minimum(2 * n, 8 * np.sqrt(n)) + 2) * U * ref["sa"] +
                                              3 * U * (np.abs(ref["G"]) + np.abs(ref["r"]))) + 1e-6 * ref["scale"]


def backward_ratio(dP, ref):
    r = np.abs(np.asarray(dP, np.float64) - ref["dP"]) / backward_bound(ref)
    return float(np.where(np.isfinite(r), r, np.inf).max()) if r.size else 0.0


# ------------------------------------------------------------------------------- data ----
def hot_positions(pat, where="mod7"):
    """The hot entry of every row (position inside the row, -1 for empty rows): (7 i) mod len, or
    min(where, len - 1) for an integer `where` counted from the row's start, "last" = len - 1."""
    lens = row_lengths(pat)
    i = np.arange(pat[0])
    if where == "mod7":
        pos = (7 * i) % np.maximum(lens, 1)
    elif where == "last":
        pos = lens - 1
    else:
        pos = np.minimum(int(where), lens - 1)
    return np.where(lens > 0, pos, -1)


def long_hot_places():
    """first, last and both sides of every pass boundary of the longest `long` row."""
    b = limits()["block_pass"]
    return [0, "last", b - 1, b, 2 * b - 1, 2 * b]


def one_hot(pat, where="mod7"):
    """(P, the one-hot W it must give, bit for bit)."""
    pos = hot_positions(pat, where)
    nnz = len(pat[3])
    P = np.full(nnz, COLD, np.float32)
    W = np.zeros(nnz, np.float32)
    live = pos >= 0
    e = np.asarray(pat[2], np.int64)[:-1][live] + pos[live]
    P[e] = HOT
    W[e] = 1.0
    return P, W


def grid_scores(pat, seed):
    return grid_data(len(pat[3]), seed)


def row_shifts(pat):
    """Per entry: +1000 on the even rows, +4096 on the odd ones (exact on the 1/8 grid)."""
    return np.where(entry_rows(pat) % 2 == 0, np.float32(1000.0), np.float32(4096.0)).astype(np.float32)


def window(pat, where):
    """(P, inside mask): per row 64 consecutive entries 0 and the rest -2000 (rows under 64: all
    0). where "tail": the row's last 64; "boundary": 32 on each side of the first pass boundary
    (rows that do not reach it: the tail)."""
    b = limits()["block_pass"]
    P = np.full(len(pat[3]), COLD, np.float32)
    rp = np.asarray(pat[2], np.int64)
    for r, n in enumerate(row_lengths(pat)):
        a = n - 64 if where == "tail" or n < b + 32 else b - 32
        P[rp[r] + max(a, 0):rp[r] + max(a, 0) + min(n, 64)] = 0.0
    return P, P == 0


def signed_scores(pat, kind, seed):
    """narrow: uniform [-1, 1); wide: uniform [-8, 8). Full mantissa."""
    return signed_data(len(pat[3]), seed) * np.float32(1.0 if kind == "narrow" else 8.0)


def backward_grid(pat, seed):
    """(W, G): W signed powers of two in [1/4, 4], G multiples of 1/8 in [-4, 4)."""
    rng = np.random.default_rng(seed)
    nnz = len(pat[3])
    W = (2.0 ** rng.integers(-2, 3, nnz) * rng.choice([-1.0, 1.0], nnz)).astype(np.float32)
    return W, grid_data(nnz, seed + 1)


def backward_signed(pat, scale, seed):
    """(W, G): W a float64 softmax of narrow scores rounded to fp32, G uniform in [-1, 1)."""
    W = softmax_ref(pat, signed_scores(pat, "narrow", seed), scale)["W"].astype(np.float32)
    return W, signed_data(len(pat[3]), seed + 1)


# -------------------------------------------------------------- expected item list ----
def lane_class(n):
    L = 1
    while L < n:
        L <<= 1
    return L


def expected_items(pat):
    """The item list as the row lengths and the exported thresholds give it: rows of one power-of-two
    class packed greedily (empty rows ride along, never at a run's end), one item per longer row."""
    w = limits()["wave_max"]
    lens, rp = row_lengths(pat), np.asarray(pat[2], np.int64)
    M, out, r = pat[0], [], 0
    while r < M:
        n = int(lens[r])
        if n == 0:
            r += 1
        elif n > 64:
            out.append((r, rp[r], n, bsmr.SOFTMAX_BLOCK if n > w else bsmr.SOFTMAX_WAVE))
            r += 1
        else:
            L, last, q = lane_class(n), r, r + 1
            while q < M and q - r < 64 // L:
                if lens[q] and (lens[q] > 64 or lane_class(int(lens[q])) != L):
                    break
                if lens[q]:
                    last = q
                q += 1
            out.append((r, rp[r], last - r + 1, L))
            r = last + 1
    return np.array(out, np.uint32).reshape(-1, 4)


def expected_stats(pat):
    it, lim = expected_items(pat), limits()
    kind = it[:, 3]
    return dict(items=len(it), packed_runs=int((kind <= 64).sum()), wave_rows=int((kind == bsmr.SOFTMAX_WAVE).sum()),
                block_rows=int((kind == bsmr.SOFTMAX_BLOCK).sum()), max_row=int(row_lengths(pat).max(initial=0)),
                wave_max=lim["wave_max"], block_pass=lim["block_pass"])


# --------------------------------------------------------------------------- emulation ----
MUTATIONS = ("drop_last_term", "neighbour_entry", "drop_last_partial", "max_without_last", "round_bf16")
INDEX_MUTATIONS = ("drop_last_term", "neighbour_entry", "drop_last_partial", "max_without_last")
LOG2E = 1.4426950408889634


def _butterfly(v, width):
    """v (..., lanes): the xor butterfly of offsets width / 2 .. 1 along the last axis, in fp32."""
    idx = np.arange(v.shape[-1])
    off = width // 2
    while off >= 1:
        v = (v + v[..., idx ^ off]).astype(np.float32)
        off //= 2
    return v


def _tile(x, T, fill):
    """A pass of len(x) <= 16 T entries as registers [T, 16]: entry k in thread (k // 4) % T,
    register 4 (k // 4 // T) + k % 4."""
    regs = np.full((T, 16), fill, np.float32)
    k = np.arange(len(x))
    regs[(k // 4) % T, 4 * (k // 4 // T) + k % 4] = x
    return regs


def _team_sum(regs, T, drop_last_partial=False, used=None):
    """Registers [T, 16] summed as the kernel does: a thread its registers in index order, a wave
    by the butterfly, the waves' partials in wave order."""
    acc = np.zeros(T, np.float32)
    for j in range(16):
        acc = (acc + regs[:, j]).astype(np.float32)
    part = _butterfly(acc.reshape(T // 64, 64), 64)[:, 0]
    if drop_last_partial and T > 64:
        part = part.copy()
        quads = -(-used // 4)  # quad q sits in thread q % T
        part[T // 64 - 1 if quads >= T else (quads - 1) // 64] = 0
    s = np.float32(0)
    for w in range(T // 64):
        s = np.float32(s + part[w])
    return s


def _exp2(x):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.exp2(x.astype(np.float32)).astype(np.float32)


def _row_forward(x, kind, c, mutation):
    """W (fp32) of one row x (fp32, already mutated where the mutation changes what is read)."""
    n = len(x)
    lim = limits()
    NINF = np.float32(-np.inf)
    xm = x[:-1] if mutation == "max_without_last" else x
    with np.errstate(invalid="ignore", over="ignore"):
        if kind <= 64:
            L = int(kind)
            lanes = np.full(L, NINF, np.float32)
            lanes[:n] = x
            m = np.float32(xm.max(initial=NINF))
            shift = np.float32(0) if m == NINF else m
            t = _exp2((lanes - shift) * c)
            tt = t.copy()
            if mutation == "drop_last_term":
                tt[n - 1] = 0
            s = _butterfly(tt, L)[0]
            inv = np.float32(0) if s == 0 else np.float32(1) / s
            return (t[:n] * inv).astype(np.float32)
        T = 64 if kind == bsmr.SOFTMAX_WAVE else lim["block_pass"] // 16
        PASS = 16 * T
        m, s, shift = NINF, np.float32(0), np.float32(0)
        for b in range(0, n, PASS):
            xp = x[b:b + PASS]
            mp = xm[b:b + PASS]
            mn = np.float32(max(m, mp.max(initial=NINF)))
            shift = np.float32(0) if mn == NINF else mn
            t = _exp2((xp - shift) * c)
            if mutation == "drop_last_term" and b + PASS >= n:
                t = t.copy()
                t[-1] = 0
            acc = _team_sum(_tile(t, T, 0.0), T, mutation == "drop_last_partial", len(xp))
            s = np.float32(s * _exp2(np.float32((m - shift) * c)) + acc) if m != NINF else acc
            m = mn
        inv = np.float32(0) if s == 0 else np.float32(1) / s
        return (_exp2((x - shift) * c) * inv).astype(np.float32)


def softmax_emulate(pat, P, scale, mutation=None):
    """W (fp32, nnz) as k_softmax_rows / k_softmax_block compute it, in numpy
    fp32 over bsmr.softmax_items: d = (P - max) * c with c = scale log2(e) rounded once from
    double, t = 2^d, a packed row summed by the butterfly of its L lanes, a wave or block row per
    thread in register order, per wave by the butterfly, waves in wave order, passes in pass
    order with the running sum rescaled by 2^((old max - new max) c); W = t * (1 / sum). numpy's
    exp2 stands in for v_exp_f32 (both within 1 ulp), so the GPU is not expected to match this
    bit for bit on general data, only where every step is exact. mutation (MUTATIONS), a wrong
    kernel for test_softmax_ref_cpu.py: "drop_last_term": a row's last term is left out of its
    sum; "neighbour_entry": a row's last lane reads the first entry of the next non-empty row;
    "drop_last_partial": a block row's sum loses the partial of the last wave that holds entries
    of the pass; "max_without_last": the maximum skips the row's last entry; "round_bf16"."""
    assert mutation is None or mutation in MUTATIONS, mutation
    P = np.asarray(P, np.float32)
    c = np.float32(np.float64(np.float32(scale)) * LOG2E)
    rp = np.asarray(pat[2], np.int64)
    W = np.full(len(P), np.nan, np.float32)
    for row, first, count, kind in bsmr.softmax_items(pat[0], pat[2]).astype(np.int64):
        rows = range(row, row + count) if kind <= 64 else [row]
        for r in rows:
            a, b = rp[r], rp[r + 1]
            if a == b:
                continue
            x = P[a:b].copy()
            if mutation == "neighbour_entry" and b < len(P):
                x[-1] = P[b]
            W[a:b] = _row_forward(x, kind, c, mutation)
    if mutation == "round_bf16":
        from gpu_util import half_values
        W = half_values(W, bsmr.BF16)
    return W


def backward_emulate(pat, W, G, scale):
    """dP (fp32) in the kernel's order: r the row's sum of W G (a packed row: rounded products by
    the butterfly; a wave or block row: one FMA per register, butterfly, waves, passes), then
    scale * (W * (G - r)), each step rounded."""
    W, G = np.asarray(W, np.float32), np.asarray(G, np.float32)
    sc = np.float32(scale)
    rp = np.asarray(pat[2], np.int64)
    lim = limits()
    out = np.full(len(W), np.nan, np.float32)
    for row, first, count, kind in bsmr.softmax_items(pat[0], pat[2]).astype(np.int64):
        for r in (range(row, row + count) if kind <= 64 else [row]):
            a, b = rp[r], rp[r + 1]
            if a == b:
                continue
            w, g = W[a:b], G[a:b]
            if kind <= 64:
                lanes = np.zeros(int(kind), np.float32)
                lanes[:b - a] = w * g
                rs = _butterfly(lanes, int(kind))[0]
            else:
                T = 64 if kind == bsmr.SOFTMAX_WAVE else lim["block_pass"] // 16
                rs = np.float32(0)
                for p0 in range(0, b - a, 16 * T):
                    tw, tg = _tile(w[p0:p0 + 16 * T], T, 0.0), _tile(g[p0:p0 + 16 * T], T, 0.0)
                    acc = np.zeros(T, np.float32)
                    for j in range(16):
                        acc = (tw[:, j].astype(np.float64) * tg[:, j] + acc).astype(np.float32)
                    part = _butterfly(acc.reshape(T // 64, 64), 64)[:, 0]
                    s = np.float32(0)
                    for x in part:
                        s = np.float32(s + x)
                    rs = np.float32(rs + s)
            out[a:b] = sc * (w * (g - rs).astype(np.float32)).astype(np.float32)
    return out


# ------------------------------------------------------------------------- the checks ----
def check_exact(W, want, pat, what):
    """W equals `want` bit for bit (both fp32); names the first rows that differ."""
    W = np.asarray(W)
    assert W.dtype == np.float32 and W.shape == want.shape, (what, W.dtype, W.shape)
    bad = np.nonzero(W.view(np.uint32) != np.asarray(want, np.float32).view(np.uint32))[0]
    if len(bad):
        rows = np.unique(entry_rows(pat)[bad])
        raise AssertionError(f"{what}: {len(bad)} entries in {len(rows)} rows differ, first rows {rows[:5]} "
                             f"(lengths {row_lengths(pat)[rows[:5]]}): got {W[bad[:4]]} want {want[bad[:4]]}")


def check_forward(W, pat, P, scale, what, kind):
    """Every entry within forward_bound of the float64 reference and every row sum within its
    bound; prints "RATIO softmax/kind ..."; returns the worst entry ratio."""
    ref = softmax_ref(pat, P, scale)
    ratio, rs = forward_ratio(W, ref), row_sum_ratio(pat, W)
    print(f"RATIO softmax/{kind} {ratio:.4f} rowsum {rs:.4f} {what}")
    assert ratio <= 1.0, f"{what}: worst |W - ref| / bound = {ratio:.3f}"
    assert rs <= 1.0, f"{what}: worst |row sum - 1| / bound = {rs:.3f}"
    return ratio


def check_window(W, pat, inside, what):
    """1/64 inside the window within the bound, exactly 0 outside."""
    P = np.where(inside, np.float32(0), COLD)
    assert (np.asarray(W)[~inside] == 0).all(), f"{what}: a weight outside the window is not exactly 0"
    ref = softmax_ref(pat, P, 1.0)
    ratio = forward_ratio(W, ref, inside)
    assert ratio <= 1.0, f"{what}: worst |W - 1/64| / bound inside the window = {ratio:.3f}"


# ------------------------------------------------------- device helpers (GPU tests only) ----
FREE = 288 * 1024 ** 3
FILL_BITS = 0x5A5AC3C3  # what an output holds before a launch: any entry left unwritten shows


def make_plan(pat):
    M, N, rp, ci = pat
    return bsmr.Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE)


def filled(n, pad=64):
    """(buffer of n + pad fp32 holding FILL_BITS, its first n)."""
    from gpu_util import torch_cuda
    torch = torch_cuda()
    buf = torch.full((max(int(n), 1) + pad,), FILL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[:max(int(n), 1)]


def dev(x):
    """x (fp32 host vector) on the device, at least one element long (a launch wants a pointer)."""
    from gpu_util import torch_cuda
    torch = torch_cuda()
    x = np.ascontiguousarray(x, np.float32)
    return torch.from_numpy(x if len(x) else np.zeros(1, np.float32)).cuda()


def _stream(stream):
    from gpu_util import torch_cuda
    return (stream or torch_cuda().cuda.current_stream()).cuda_stream


def softmax_once(plan, P, scale):
    """W (numpy fp32, nnz) of one bsmr_softmax on host scores. W starts as FILL_BITS: the launch
    must write every entry and nothing behind the last."""
    from gpu_util import torch_cuda
    torch = torch_cuda()
    buf, dW = filled(len(P))
    dP = dev(P)  # (kept alive across the launch)
    plan.softmax(dP.data_ptr(), dW.data_ptr(), scale, stream=_stream(None))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[max(len(P), 1):].view(np.uint32) == FILL_BITS).all(), "a store past the last entry"
    W = host[:len(P)]
    assert not (W.view(np.uint32) == FILL_BITS).any(), "an entry was never written"
    return W


def backward_once(plan, W, G, scale):
    from gpu_util import torch_cuda
    torch = torch_cuda()
    buf, dGP = filled(len(W))
    dW, dG = dev(W), dev(G)  # (kept alive across the launch)
    plan.softmax_backward(dW.data_ptr(), dG.data_ptr(), dGP.data_ptr(), scale, stream=_stream(None))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[max(len(W), 1):].view(np.uint32) == FILL_BITS).all(), "a store past the last entry"
    out = host[:len(W)]
    assert not (out.view(np.uint32) == FILL_BITS).any(), "an entry was never written"
    return out
