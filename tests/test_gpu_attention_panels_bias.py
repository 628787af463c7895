"""The panel MFMA attention with a per-entry additive bias against exact and
float64 references on small patterns and the transposes that split the columns side.

Bounds of test_against_float64, on the biased float64 reference; u = 2^-24, u_T = 2^-11 (fp16) or 2^-8 (bf16), s the
steps of a row's panel, ex = 2 u (|p scale| + |bias|) the two extra roundings of x, entering as a score error does:
  O: attention_bound + sum 2 W max_row(ex) |V| + section 18's u_T A + s u A (+ n 2^-25 max |V|, fp16), A = sum W |V|;
  LSE: lse_bound + max_row(ex) (log-sum-exp is 1-Lipschitz) + 3 s u;
  GQ, GK, GV: backward_bound + the sums of dw_x = w ex (GV) and scale dw_x |g - delta| (GQ, GK) + section 19's terms:
  |dg| <= u_T S_g (GO rounded once; + Dv 2^-25 max |V|, fp16) reaching dp as scale w dg, u_T |dp|, (2 u_T + u_T^2)
  sum w |GO|, and in fp16 2^-25 per factor that can fall under 2^-14 times the largest other factor, per term;
  GBias: (entry_bounds' ddp + scale dw_x |g - delta|) / scale + w dg: dp before its product with scale, kept in fp32.
"""
import functools

import numpy as np
import pytest

import attention_bwd_cases as ABC
import attention_cases as AC
import bsmr
from attention_bwd_cases import _dst_sums
from attention_cases import FILL_BITS, filled
from bsmr import BF16, F16, F32
from gpu_util import half_values, to_device, torch_cuda
from sddmm_cases import grid_data

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED, U = 1, 6, 2.0 ** -24
FORMS = [pytest.param(dt, D, Dv, id=f"{AC.DTYPE_NAME[dt]}-{D}-{Dv}") for dt in (F16, BF16)
         for D, Dv in [(32, 32), (64, 128), (128, 64)]]
PATTERNS = ["staircase37", "union_32_33", "empty_row_and_panel", "split", "hub", "staircase37_T", "split_T"]
OUT = ("GQ", "GK", "GV", "GBias")


_stream = lambda: torch_cuda().cuda.current_stream().cuda_stream  # noqa: E731


def _groups(groups, N):
    """Rows given as (count, columns) groups: `count` rows storing exactly `columns`."""
    lens = np.concatenate([[len(c)] * n for n, c in groups])
    ci = np.concatenate([np.tile(np.asarray(c, np.uint32), n) for n, c in groups])
    return len(lens), N, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32), ci.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def pattern(name):
    r, n = np.arange, bsmr.attention_panels_limits()["item_steps"] * 32 + 1
    if name.endswith("_T"):
        return ABC.transpose(pattern(name[:-2]))
    return {"staircase37": lambda: _groups([(1, r(i + 1)) for i in range(37)], 40),  # a short last panel, a second step
            "union_32_33": lambda: _groups([(16, r(32)), (16, r(40, 73))], 80),  # one full step; a step and a column
            "empty_row_and_panel": lambda: _groups([(7, r(3, 23)), (1, []), (8, r(3, 23)), (16, [])], 32),
            "split": lambda: _groups([(16, r(n)), (5, r(7))], n + 3),  # a union of one item and a column: two items
            "hub": lambda: AC.pattern("hub")}[name]()


@functools.lru_cache(maxsize=None)
def plan_of(name):
    return AC.make_plan(pattern(name))


def _read(buf, n, shape, what):
    h = buf.cpu().numpy()
    assert (h[n:].view(np.uint32) == FILL_BITS).all(), f"a store past the end of {what}"
    assert not (h[:n].view(np.uint32) == FILL_BITS).any(), f"an element of {what} was never written"
    return h[:n].reshape(shape)


def forward(plan, dev, bias, D, Dv, scale, dtype):
    """(O, LSE) of one biased forward on device operands (Q, K, V, ...); outputs start as FILL_BITS."""
    bufO, dO = filled(plan.M * Dv)
    bufL, dL = filled(plan.M)
    plan.attention_panels_bias(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), bias.data_ptr(), D, Dv, dO.data_ptr(),
                               dL.data_ptr(), scale, stream=_stream(), dtype=dtype)
    torch_cuda().cuda.synchronize()
    return _read(bufO, plan.M * Dv, (plan.M, Dv), "O"), _read(bufL, plan.M, (plan.M,), "LSE")


def backward(plan, dev, bias, D, Dv, scale, dtype, want=OUT):
    """dict(GQ, GK, GV, GBias) of one biased backward on ABC.device_inputs operands (None: not in `want`)."""
    shapes = dict(GQ=(plan.M, D), GK=(plan.N, D), GV=(plan.N, Dv), GBias=(plan.nnz,))
    bufs = {k: filled(int(np.prod(s))) for k, s in shapes.items()}
    ptr = [bufs[k][1].data_ptr() if k in want else 0 for k in OUT]
    plan.attention_backward_panels_bias(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), bias.data_ptr(),
                                        *(t.data_ptr() for t in dev[3:]), D, Dv, *ptr, scale, stream=_stream(), dtype=dtype)
    torch_cuda().cuda.synchronize()
    out = {}
    for k, s in shapes.items():
        if k in want:
            out[k] = _read(bufs[k][0], int(np.prod(s)), s, k)
        else:
            assert (bufs[k][0].cpu().numpy().view(np.uint32) == FILL_BITS).all(), f"{k} written though it was not asked for"
            out[k] = None
    return out


def same(a, b):  # two result dicts, bit for bit
    return all((a[k] is None and b[k] is None) or bool((a[k].view(np.uint32) == b[k].view(np.uint32)).all()) for k in a)


def biased_ref(pat, ops, bias, scale, dtype):
    """ABC.backward_ref with the definition's x = p scale + bias, w = exp(x - LSE) (0 for bias = -inf or LSE = -inf),
    GBias = h = w (g - delta), dp = h scale and the float64 GQ, GK, GV of those."""
    ref = ABC.backward_ref(pat, *ops, scale, dtype)
    rows, cols, M, N = ref["rows"], ref["cols"], ref["M"], ref["N"]
    with np.errstate(invalid="ignore", over="ignore"):
        x = ref["p"] * scale + bias.astype(np.float64)
        w = np.where((ref["lse"] == -np.inf) | (x == -np.inf), 0.0, np.exp(x - np.where(ref["lse"] == -np.inf, 0.0, ref["lse"])))
        h = w * ref["gd"]
    dp = h * scale
    return dict(ref, GQ=_dst_sums(M, rows, dp, ref["K"], cols), GK=_dst_sums(N, cols, dp, ref["Q"], rows),
                GV=_dst_sums(N, cols, w, ref["GO"], rows), GBias=h, x=x, w=w, dp=dp)


def forward_ref(pat, Q, K, V, bias, scale, dtype):
    """AC.attention_ref with the softmax of x = p scale + bias: W, d, sd, l, LSE, O, and m in p's units (m scale = max x)."""
    f = AC.attention_ref(pat, Q, K, V, scale, dtype)
    x = f["p"] * scale + bias
    mx, l = np.full(pat[0], -np.inf), np.zeros(pat[0])
    np.maximum.at(mx, f["rows"], x)
    np.add.at(l, f["rows"], np.exp(x - mx[f["rows"]]))
    sm = AC.SC.softmax_ref(pat, x, 1.0)
    with np.errstate(divide="ignore"):
        return dict(f, W=sm["W"], d=sm["d"], sd=sm["sd"], m=mx / scale, l=l, LSE=mx + np.log(l),
                    O=AC._row_sums(pat[0], pat[2], f["cols"], sm["W"], f["V"]))


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_against_float64(dtype, D, Dv, name):
    pat, plan = pattern(name), plan_of(name)
    M, N, rp, ci = pat
    prow, _, _, items, _ = bsmr.attention_panel_lists(M, N, rp, ci, plan.array("reorderedRows"))
    steps, s = np.zeros(M), np.empty(M)  # per panel, then per row, the steps of its panel
    np.add.at(steps, items[:, 0] // 16, items[:, 2])
    s[prow] = steps[np.arange(M) // 16]
    uT, sub = (2.0 ** -11, 2.0 ** -25) if dtype == F16 else (2.0 ** -8, 0.0)
    bias = (4 * np.random.default_rng(11).random(plan.nnz) - 2).astype(np.float32)
    dB = to_device(bias, F32)
    GO = AC.signed_data(M * Dv, 14).reshape(M, Dv)
    for kind, scale in (("narrow", 1.0), ("wide", 1.0), ("narrow", D ** -0.5), ("wide", D ** -0.5)):
        Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, kind, scale)
        f = forward_ref(pat, Q, K, V, bias, scale, dtype)
        O, LSE = forward(plan, [to_device(X, dtype) for X in (Q, K, V)], dB, D, Dv, scale, dtype)
        exmax = AC._row_max(f, 2 * U * (np.abs(f["p"] * scale) + np.abs(bias)))
        A, n = AC._weighted(f, f["W"]), f["lens"].astype(np.float64)[:, None]
        bO = (AC.attention_bound(f, opscale) + AC._weighted(f, 2 * f["W"] * exmax[f["rows"]]) + (uT + s[:, None] * U) * A +
              n * sub * np.abs(f["V"]).max())
        live = f["lens"] > 0
        assert (O[~live] == 0).all() and (LSE[~live] == -np.inf).all()
        r = dict(O=AC._ratio(np.abs(O - f["O"]), bO),
                 LSE=AC._ratio(np.abs(LSE[live] - f["LSE"][live]), (AC.lse_bound(f, opscale) + exmax + 3 * s * U)[live]))
        ops = (Q, K, V, f["O"].astype(np.float32), GO, f["LSE"].astype(np.float32))
        b = biased_ref(pat, ops, bias, scale, dtype)
        got = backward(plan, ABC.device_inputs(*ops, dtype), dB, D, Dv, scale, dtype)
        rows, cols, w = b["rows"], b["cols"], b["w"]
        aK, aQ, aGO = np.abs(b["K"]), np.abs(b["Q"]), np.abs(b["GO"])
        dw, ddp = ABC.entry_bounds(b, opscale)
        dwx = w * 2 * U * (np.abs(b["p"] * scale) + np.abs(bias))
        dg = uT * b["Sg"] + Dv * sub * np.abs(b["V"]).max()
        ddpx = scale * dwx * np.abs(b["gd"])
        e = ddpx + scale * w * dg + uT * np.abs(b["dp"])  # per entry, what backward_bound's ddp does not hold
        rl, cl = b["rlen"].astype(np.float64)[:, None], b["clen"].astype(np.float64)[:, None]
        base = ABC.backward_bound(b, opscale)
        bound = dict(GQ=base["GQ"] + _dst_sums(M, rows, e, aK, cols) + rl * sub * aK.max(initial=0),
                     GK=base["GK"] + _dst_sums(N, cols, e, aQ, rows) + cl * sub * aQ.max(initial=0),
                     GV=base["GV"] + _dst_sums(N, cols, dwx + (2 * uT + uT * uT) * w, aGO, rows) +
                     cl * sub * (aGO.max(initial=0) + w.max(initial=0)), GBias=(ddp + ddpx) / scale + w * dg)
        r.update({k: AC._ratio(np.abs(got[k] - b[k]), bound[k]) for k in OUT})
        print(f"RATIO attention_panels_bias {AC.DTYPE_NAME[dtype]} {D} {Dv} {name} {kind} {scale:.4f}: " +
              " ".join(f"{k} {v:.4f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0, (kind, scale, r)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_forward_selects_the_unmasked_entry_bit_for_bit(dtype, D, Dv, name):
    # Q = 0, so x is the bias: 0 at one winner per row and -inf elsewhere gives w = 1 there, O = V[winner]
    # and LSE = 0 exactly; the row whose entries are all -inf is an empty row
    pat, plan = pattern(name), plan_of(name)
    M, N, rp, ci = pat
    lens = AC.row_lengths(pat)  # the winner: the middle entry of every row but the last live one, which keeps none
    win = np.where(lens > 0, np.asarray(rp[:-1], np.int64) + lens // 2, -1)
    dead = int(np.nonzero(lens)[0][-1])
    win[dead] = -1
    bias = np.full(max(len(ci), 1), -np.inf, np.float32)
    bias[win[win >= 0]] = 0.0
    V = grid_data(N * Dv, 7).reshape(N, Dv)
    dev = [to_device(X, dtype) for X in (np.zeros((M, D), np.float32), AC.signed_data(N * D, 5).reshape(N, D), V)]
    for scale in (1.0, 0.125):
        O, LSE = forward(plan, dev, to_device(bias, F32), D, Dv, scale, dtype)
        wantO = np.where((win >= 0)[:, None], half_values(V, dtype)[np.asarray(ci, np.int64)[np.maximum(win, 0)]], np.float32(0))
        AC.check_exact(O, wantO, f"O {name}")
        AC.check_exact(LSE, np.where(win >= 0, np.float32(0), np.float32(-np.inf)), f"LSE {name}")
        assert (O[dead] == 0).all() and LSE[dead] == -np.inf


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_backward_flat_set_is_bit_exact(dtype, D, Dv, name):
    # section 14's flat set (p = 0, so x is the bias) with a constant bias 0.5 and LSE = 0.5: w = 1 exactly;
    # every third entry is removed by bias = -inf (w = 0, GBias = 0)
    pat, plan = pattern(name), plan_of(name)
    ops = list(ABC.flat_inputs(pat, D, Dv, dtype))
    ops[5] = np.full(pat[0], 0.5, np.float32)
    bias = np.full(max(len(pat[3]), 1), 0.5, np.float32)
    bias[::3] = -np.inf
    ref = biased_ref(pat, ops, bias[:len(pat[3])], 0.5, dtype)
    for X in (ops[4], ref["w"], ref["dp"]):  # GO, w, dp: the rounding to the operand type changes nothing
        assert (half_values(X, dtype).astype(np.float64) == X).all()
    got = backward(plan, ABC.device_inputs(*ops, dtype), to_device(bias, F32), D, Dv, 0.5, dtype)
    for k in OUT:
        want = ref[k].astype(np.float32)
        assert (want.astype(np.float64) == ref[k]).all(), f"the reference {k} is not an fp32 value"
        # (a removed entry's GBias is 0 x (g - delta): a zero of either sign)
        AC.check_exact((got[k] + np.float32(0)).reshape(len(want), -1), (want + np.float32(0)).reshape(len(want), -1), f"{k} {name}")


def _signed(name, D, Dv, dtype, scale=0.125, seed=11):
    """Signed operands with the biased forward's own O and LSE, on the device, and the bias in [-2, 2]."""
    pat, plan = pattern(name), plan_of(name)
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "narrow", scale, seed)
    bias = (4 * np.random.default_rng(seed).random(max(plan.nnz, 1)) - 2).astype(np.float32)
    dev = [to_device(X, dtype) for X in (Q, K, V)]
    dB = to_device(bias, F32)
    O, LSE = forward(plan, dev, dB, D, Dv, scale, dtype)
    GO = AC.signed_data(pat[0] * Dv, seed + 3).reshape(pat[0], Dv)
    return (Q, K, V, O, GO, LSE), ABC.device_inputs(Q, K, V, O, GO, LSE, dtype), bias, dB


@pytest.mark.parametrize("dtype,D,Dv,name", [(F16, 64, 128, "split"), (BF16, 32, 32, "split_T")])
def test_bitwise_properties(dtype, D, Dv, name):
    torch = torch_cuda()
    pat, plan = pattern(name), AC.make_plan(pattern(name))  # a fresh plan, built lazily by its first launch
    ops, dev, _, dB = _signed(name, D, Dv, dtype)
    q, k, v = dev[:3]

    def unbiased(p):
        bufO, dO = filled(p.M * Dv)
        p.attention_panels(q.data_ptr(), k.data_ptr(), v.data_ptr(), D, Dv, dO.data_ptr(), 0, 0.125, stream=_stream(), dtype=dtype)
        torch.cuda.synchronize()
        return bufO.cpu().numpy()

    before = unbiased(plan)
    fwd = forward(plan, dev, dB, D, Dv, 0.125, dtype)
    full = backward(plan, dev, dB, D, Dv, 0.125, dtype)
    assert (unbiased(plan).view(np.uint32) == before.view(np.uint32)).all(), "a biased launch changed the unbiased result"
    prepared = AC.make_plan(pat)
    prepared.prepare_attention_panels_bias(D, Dv)
    prepared.prepare_attention_panels_bias(D, Dv, backward=True)
    assert prepared.attention_panels_bias_prepared(D, Dv) and prepared.attention_panels_bias_prepared(D, Dv, backward=True)
    assert all((a.view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(fwd, forward(prepared, dev, dB, D, Dv, 0.125, dtype)))
    assert same(full, backward(prepared, dev, dB, D, Dv, 0.125, dtype)), "prepared and lazy plans differ"
    for want in (("GBias",), ("GQ", "GBias"), ("GK", "GV"), ("GQ",)):
        part = backward(plan, dev, dB, D, Dv, 0.125, dtype, want=want)
        assert all((part[x].view(np.uint32) == full[x].view(np.uint32)).all() for x in want), want
    # a graph of the prepared plan's forward and backward, replayed, against the eager results
    bufs = [filled(n)[1] for n in (plan.M * Dv, plan.M, plan.M * D, plan.N * D, plan.N * Dv, plan.nnz)]
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = side.cuda_stream
        prepared.attention_panels_bias(q.data_ptr(), k.data_ptr(), v.data_ptr(), dB.data_ptr(), D, Dv, bufs[0].data_ptr(),
                                       bufs[1].data_ptr(), 0.125, stream=s, dtype=dtype)
        prepared.attention_backward_panels_bias(q.data_ptr(), k.data_ptr(), v.data_ptr(), dB.data_ptr(), dev[3].data_ptr(),
                                                dev[4].data_ptr(), dev[5].data_ptr(), D, Dv, *(b.data_ptr() for b in bufs[2:]),
                                                0.125, stream=s, dtype=dtype)
    for _ in range(3):
        for b in bufs:
            b.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for b, e in zip(bufs, list(fwd) + [full[x] for x in OUT]):
            assert (b.cpu().numpy().view(np.uint32) == e.ravel().view(np.uint32)).all(), "a replay differs from the eager call"


@pytest.mark.parametrize("dtype,D,Dv,name,shared", [(F16, 64, 128, "hub", True), (BF16, 32, 32, "split_T", False)])
def test_heads_slices_equal_the_single_slice_call(dtype, D, Dv, name, shared):
    torch = torch_cuda()
    B, H = 2, 2
    pat, plan = pattern(name), plan_of(name)
    M, N, nnz, s = pat[0], pat[1], plan_of(name).nnz, _stream()
    tdt = torch.float16 if dtype == F16 else torch.bfloat16
    data = lambda n, seed, t=tdt: torch.from_numpy(AC.signed_data(n, seed)).to(t).cuda()  # noqa: E731
    Q = data(B * M * H * D, 1).view(B, M, H, D).transpose(1, 2)  # a view of a (B, M, H D) projection
    K = data(B * N * D, 2).view(B, 1, N, D).expand(B, H, N, D)   # one K / V for all heads: head stride 0
    V = data(B * N * Dv, 3).view(B, 1, N, Dv).expand(B, H, N, Dv)
    GO = data(B * H * M * Dv, 4, torch.float32).view(B, H, M, Dv)
    bias = data((1 if shared else B * H) * (nnz + 4), 5, torch.float32).view(-1, nnz + 4)  # (a stride above nnz)
    bstride = 0 if shared else nnz + 4
    O, L = torch.empty(B, H, M, Dv, device="cuda"), torch.empty(B, H, M, device="cuda")
    plan.attention_panels_bias_heads(B, H, Q, K, V, bias.data_ptr(), bstride, D, Dv, O, L.data_ptr(), 0.25, stream=s, dtype=dtype)
    GQ = torch.full((B, M, H, D), float("nan"), device="cuda").transpose(1, 2)
    GK, GV = torch.full((B, H, N, D), float("nan"), device="cuda"), torch.full((B, H, N, Dv), float("nan"), device="cuda")
    GB = torch.full((B * H, nnz + 8), float("nan"), device="cuda")
    plan.attention_backward_panels_bias_heads(B, H, Q, K, V, bias.data_ptr(), bstride, O, GO, L.data_ptr(), D, Dv, GQ, GK, GV,
                                              GB.data_ptr(), nnz + 8, 0.25, stream=s, dtype=dtype)
    assert torch.isnan(GB[:, nnz:]).all(), "a GBias store between the slices"
    for b in range(B):
        for h in range(H):
            q, k, v = (X[b, h].contiguous() for X in (Q, K, V))
            bs = bias[0 if shared else b * H + h].contiguous()
            o, l = torch.empty(M, Dv, device="cuda"), torch.empty(M, device="cuda")
            plan.attention_panels_bias(q.data_ptr(), k.data_ptr(), v.data_ptr(), bs.data_ptr(), D, Dv, o.data_ptr(), l.data_ptr(),
                                       0.25, stream=s, dtype=dtype)
            assert torch.equal(O[b, h], o) and torch.equal(L[b, h], l), (b, h)
            gq, gk, gv, gb = (torch.empty(n, w, device="cuda") for n, w in ((M, D), (N, D), (N, Dv), (1, nnz)))
            plan.attention_backward_panels_bias(q.data_ptr(), k.data_ptr(), v.data_ptr(), bs.data_ptr(), o.data_ptr(),
                                                GO[b, h].data_ptr(), l.data_ptr(), D, Dv, gq.data_ptr(), gk.data_ptr(),
                                                gv.data_ptr(), gb.data_ptr(), 0.25, stream=s, dtype=dtype)
            assert torch.equal(GQ[b, h], gq) and torch.equal(GK[b, h], gk) and torch.equal(GV[b, h], gv), (b, h)
            assert torch.equal(GB[b * H + h, :nnz], gb[0]), (b, h)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_nan_bias_stays_in_its_row(dtype):
    name, D, Dv, i = "hub", 64, 64, 5
    pat, plan = pattern(name), plan_of(name)
    M, N, rp, ci = pat
    ops, dev, bias, dB = _signed(name, D, Dv, dtype)
    cleanF, clean = forward(plan, dev, dB, D, Dv, 0.125, dtype), backward(plan, dev, dB, D, Dv, 0.125, dtype)
    bad = bias.copy()
    bad[rp[i]] = np.nan
    dBad = to_device(bad, F32)
    O, LSE = forward(plan, dev, dBad, D, Dv, 0.125, dtype)
    others = np.arange(M) != i
    assert np.isnan(O[i]).all() and np.isnan(LSE[i])
    assert (O[others].view(np.uint32) == cleanF[0][others].view(np.uint32)).all() and (LSE[others] == cleanF[1][others]).all()
    got = backward(plan, ABC.device_inputs(*ops[:3], O, ops[4], LSE, dtype), dBad, D, Dv, 0.125, dtype)
    stored = np.zeros(N, bool)
    stored[ci[rp[i]:rp[i + 1]]] = True
    mine = AC.entry_rows(pat) == i
    assert np.isnan(got["GQ"][i]).all() and np.isnan(got["GBias"][mine]).all()
    assert (got["GQ"][others].view(np.uint32) == clean["GQ"][others].view(np.uint32)).all()
    assert (got["GBias"][~mine].view(np.uint32) == clean["GBias"][~mine].view(np.uint32)).all()
    for k in ("GK", "GV"):
        assert np.isnan(got[k][stored]).any(axis=1).all()
        assert (got[k][~stored].view(np.uint32) == clean[k][~stored].view(np.uint32)).all(), k


def test_refusals_leave_the_outputs_untouched():
    torch = torch_cuda()
    name, D, Dv, dtype = "split", 64, 32, F16
    plan = AC.make_plan(pattern(name))  # a fresh plan: nothing prepared
    _, dev, _, dB = _signed(name, D, Dv, dtype)
    bufs = [filled(n) for n in (plan.M * Dv, plan.M, plan.M * D, plan.N * D, plan.N * Dv, plan.nnz)]
    ptr = [b[1].data_ptr() for b in bufs]
    q, k, v, o, go, lse = (t.data_ptr() for t in dev)

    def fwd(s, b=dB.data_ptr(), D_=D, dt=dtype):
        plan.attention_panels_bias(q, k, v, b, D_, Dv, ptr[0], ptr[1], 0.125, stream=s, dtype=dt)

    def bwd(s, b=dB.data_ptr(), D_=D, dt=dtype, outs=ptr[2:]):
        plan.attention_backward_panels_bias(q, k, v, b, o, go, lse, D_, Dv, *outs, 0.125, stream=s, dtype=dt)

    def status(fn, s, **kw):
        with pytest.raises(bsmr.BsmrError) as ei:
            fn(s, **kw)
        return ei.value.status

    def untouched():
        torch.cuda.synchronize()
        return all((b[0].cpu().numpy().view(np.uint32) == FILL_BITS).all() for b in bufs)

    s0 = _stream()
    for fn in (fwd, bwd):
        assert [status(fn, s0, b=0), status(fn, s0, b=dB.data_ptr() + 2)] == [INVALID] * 2, "a null or misaligned bias"
        assert [status(fn, s0, dt=F32), status(fn, s0, D_=48), status(fn, s0, D_=256)] == [UNSUPPORTED] * 3
    assert [status(bwd, s0, outs=[0, 0, 0, 0]), status(bwd, s0, outs=[0, 0, 0, ptr[5] + 2])] == [INVALID] * 2  # none; misaligned
    ops = [bsmr.AttentionOperand.of(t.view(1, *t.shape)) for t in (dev[0], dev[1], dev[2], dev[3], dev[4])]
    for bstride, gstride in ((0, 0), (plan.nnz - 1, plan.nnz)):  # a GBias stride of 0, and a bias stride under nnz
        with pytest.raises(bsmr.BsmrError) as ei:
            plan.attention_backward_panels_bias_heads(1, 1, *ops[:3], dB.data_ptr(), bstride, ops[3], ops[4], lse, D, Dv, None,
                                                      None, None, ptr[5], gstride, 0.125, stream=s0, dtype=dtype)
        assert ei.value.status == INVALID and untouched()
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        refused = [status(fwd, side.cuda_stream), status(bwd, side.cuda_stream)]
    assert refused == [bsmr.NOT_PREPARED] * 2 and untouched()
    assert not plan.attention_panels_bias_prepared(D, Dv) and not plan.attention_panels_bias_prepared(D, Dv, backward=True)


def _dense(pat, Q, K, V, b, dO, scale, dt):
    """(O, dQ, dK, dV, db) of dense masked attention with a bias in numpy at precision dt."""
    M, N, rp, ci = pat
    rows, cols = AC.entry_rows(pat), np.asarray(ci, np.int64)
    Q, K, V, dO = (np.asarray(x, dt) for x in (Q, K, V, dO))
    X = np.full((M, N), -np.inf, dt)
    X[rows, cols] = (Q @ K.T)[rows, cols] * dt(scale) + np.asarray(b, dt)
    m = X.max(axis=1, keepdims=True)
    T = np.exp(X - np.where(np.isfinite(m), m, dt(0)))
    den = T.sum(axis=1, keepdims=True)
    W = T / np.where(den == 0, dt(1), den)
    O = W @ V
    dW = dO @ V.T
    dX = W * (dW - (W * dW).sum(axis=1, keepdims=True))
    return O, dX @ K * dt(scale), dX.T @ Q * dt(scale), W.T @ dO, dX[rows, cols]


def test_autograd_against_dense_float64_attention():
    # tolerance: 8 x the error of the same dense attention computed in float16 on the CPU, against float64
    torch = torch_cuda()
    from bsmr import autograd
    pat = AC.pattern("zipf_shuffled")
    plan = AC.make_plan(pat)
    M, N, D = pat[0], pat[1], 64
    Q, K, V, dO = (half_values(AC.signed_data(r * D, 81 + n).reshape(r, D), F16) for n, r in enumerate((M, N, N, M)))
    b = (4 * np.random.default_rng(9).random(plan.nnz) - 2).astype(np.float32)
    ref = _dense(pat, Q, K, V, b, dO, D ** -0.5, np.float64)
    cpu = _dense(pat, Q, K, V, b, dO, D ** -0.5, np.float16)
    tQ, tK, tV = (torch.from_numpy(X).to(torch.float16).cuda().requires_grad_(True) for X in (Q, K, V))
    tb = torch.from_numpy(b).cuda().requires_grad_(True)
    for kw in (dict(forward="gather", backward="panels"), dict(forward="panels", backward="fused"), dict(forward="panels")):
        with pytest.raises(ValueError):
            autograd.attention_fused(plan, tQ, tK, tV, bias=tb, **kw)
    O = autograd.attention_fused(plan, tQ, tK, tV, forward="panels", backward="panels", bias=tb)
    O.backward(torch.from_numpy(dO).cuda())
    torch.cuda.synchronize()
    for what, g, r, c in zip(("O", "dQ", "dK", "dV", "dbias"), (O.detach(), tQ.grad, tK.grad, tV.grad, tb.grad), ref, cpu):
        top = np.abs(r).max()
        cpu_err = np.abs(c.astype(np.float64) - r).max() / top
        gpu_err = np.abs(g.float().cpu().numpy().astype(np.float64) - r).max() / top
        print(f"ATTENTION_PANELS_BIAS_AUTOGRAD f16 {what}: float16 CPU error {cpu_err:.3e}, GPU error {gpu_err:.3e}")
        assert 0 < cpu_err and gpu_err <= 8 * cpu_err, what
    # heads: a bias shared by the slices gets the sum of the slices' gradients
    hQ, hK, hV = (X.detach().expand(2, *X.shape).contiguous().requires_grad_(True) for X in (tQ, tK, tV))
    hb = tb.detach().clone().requires_grad_(True)
    Oh = autograd.attention_fused_heads(plan, hQ, hK, hV, forward="panels", backward="panels", bias=hb)
    Oh.backward(torch.from_numpy(dO).cuda().expand(2, M, D))
    assert torch.equal(Oh[0], O.detach()) and torch.equal(Oh[1], O.detach()) and torch.equal(hb.grad, tb.grad + tb.grad)
