"""Slices, layouts and device helpers of the fused sparse attention over batch and heads
(bsmr_attention_heads, bsmr_attention_backward_heads). Built on attention_cases
and attention_bwd_cases by import only: the float64 references, the exact data sets and the bounds
are theirs, unchanged, applied per slice. test_gpu_attention_heads_float64.py,
test_gpu_attention_heads_edges.py and test_gpu_far_attention_heads.py use this module.

Slices: slice z = b H + h of a (B, H) call has its own seed (SEED0 + SEED_STEP z), so that the
selector data has a different permutation (different winners) and the signed data different values
per slice: a slice that reads another's operand, scratch, delta or LSE cannot pass. With the
"kv_shared" layout K and V of slice (b, h) are those of slice (b, 0) (a head stride of 0); Q, GO and
what follows from them stay the slice's own.

Layouts (LAYOUTS) of a (B, H, rows, W) operand:
  bhmd       dense, standard order
  bmhd       dense (B, rows, H, W): head stride W, row stride H W
  padded     bhmd with a row stride of W + PAD; input padding holds NaN, output padding FILL_BITS
  kv_shared  K and V with head stride 0 (one (B, 1, N, W) tensor expanded), everything else bhmd
Outputs start as FILL_BITS with a guard zone behind them; read_output checks that every element of
every slice was written, that nothing behind the last element and nothing of the padding changed.
"""
import functools

import numpy as np

import attention_bwd_cases as BC
import attention_cases as AC
from attention_cases import DTYPE_NAME, FILL_BITS, check_exact  # noqa: F401
from bsmr import BF16, F16, F32  # noqa: F401

LAYOUTS = ("bhmd", "bmhd", "padded", "kv_shared")
PAD = 8  # elements: 32 bytes of fp32, 16 bytes of fp16 / bf16
GUARD = 64
SEED0, SEED_STEP = 100, 16  # (a data set uses seed .. seed + 4)
FWD_PATTERNS = ["long4", "hub", "empty"]
BWD_PATTERNS = FWD_PATTERNS + ["long4_T", "hub_T"]
# one generic and one compile-time lane form per dtype
SHAPES = [(F32, 32, 48), (F32, 64, 64), (F16, 64, 64), (BF16, 32, 128)]
BH = [(1, 3), (2, 2)]
OUTPUTS = BC.OUTPUTS


def seeds(B, H, layout):
    """[(seed of Q / GO, seed of K / V)] per slice z = b H + h."""
    out = []
    for b in range(B):
        for h in range(H):
            sq = SEED0 + SEED_STEP * (b * H + h)
            out.append((sq, SEED0 + SEED_STEP * b * H if layout == "kv_shared" else sq))
    return out


@functools.lru_cache(maxsize=None)
def plan_of(name):
    """One plan per pattern for the whole run (launches of one plan are ordered by the tests)."""
    return BC.make_plan(BC.pattern(name))


# ------------------------------------------------------------------------- slice data ----
@functools.lru_cache(maxsize=256)
def forward_slice(kind, name, D, Dv, dtype, scale, sq, skv):
    """dict(Q, K, V, and for "selector" O, LSE: what the launch must give bit for bit; for "signed"
    opscale) of one slice: Q by seed sq, K and V by seed skv."""
    pat = BC.pattern(name)
    if kind == "selector":
        Q = AC.selector(pat, D, Dv, "random", dtype, sq)[0]
        _, K, V, winner, pi, base = AC.selector(pat, D, Dv, "random", dtype, skv)
        O, LSE = AC.selector_expected(V, winner, pi, base, scale, dtype)
        return dict(Q=Q, K=K, V=V, O=O, LSE=LSE)
    assert kind == "signed"
    Q, _, _, opscale = AC.signed_inputs(pat, D, Dv, "wide", scale, sq)
    _, K, V, _ = AC.signed_inputs(pat, D, Dv, "wide", scale, skv)
    return dict(Q=Q, K=K, V=V, opscale=opscale)


@functools.lru_cache(maxsize=256)
def backward_slice(kind, name, D, Dv, dtype, scale, sq, skv):
    """dict(Q, K, V, O, GO, LSE, and for the exact kinds "selector" and "flat" GQ, GK, GV: the
    float64 answer as fp32; for "signed" opscale) of one slice."""
    pat = BC.pattern(name)
    if kind == "selector":
        GO = BC.selector_inputs(pat, D, Dv, "random", scale, dtype, sq)[4]
        Q, K, V, O, _, LSE, winner = BC.selector_inputs(pat, D, Dv, "random", scale, dtype, skv)
        GQ, GK, GV = BC.selector_expected(pat, GO, winner, D, Dv)
        return dict(Q=Q, K=K, V=V, O=O, GO=GO, LSE=LSE, GQ=GQ, GK=GK, GV=GV)
    if kind == "flat":
        Q, _, _, O, GO, LSE = BC.flat_inputs(pat, D, Dv, dtype, sq)
        _, K, V, _, _, _ = BC.flat_inputs(pat, D, Dv, dtype, skv)
        ref = BC.backward_ref(pat, Q, K, V, O, GO, LSE, scale, dtype)
        out = dict(Q=Q, K=K, V=V, O=O, GO=GO, LSE=LSE)
        for k in OUTPUTS:
            want = ref[k].astype(np.float32)
            assert (want.astype(np.float64) == ref[k]).all(), f"the flat reference {k} is not an fp32 value"
            out[k] = want + np.float32(0)
        return out
    assert kind == "signed"
    Q, _, _, opscale = AC.signed_inputs(pat, D, Dv, "wide", scale, sq)
    _, K, V, _ = AC.signed_inputs(pat, D, Dv, "wide", scale, skv)
    fwd = AC.attention_ref(pat, Q, K, V, scale, dtype)
    GO = BC.signed_data(pat[0] * Dv, sq + 3).reshape(pat[0], Dv)
    return dict(Q=Q, K=K, V=V, O=fwd["O"].astype(np.float32), GO=GO, LSE=fwd["LSE"].astype(np.float32), opscale=opscale)


def stack(slices, key):
    return np.stack([s[key] for s in slices])


@functools.lru_cache(maxsize=256)
def single_forward(name, D, Dv, dtype, scale, sq, skv, kind="signed"):
    """(O, LSE) of the existing single-slice call (attention_cases.attention_once) on a contiguous
    copy of the slice, on the shared plan."""
    s = forward_slice(kind, name, D, Dv, dtype, scale, sq, skv)
    return AC.attention_once(plan_of(name), s["Q"], s["K"], s["V"], scale, dtype)


@functools.lru_cache(maxsize=256)
def single_backward(name, D, Dv, dtype, scale, sq, skv, kind="signed"):
    """dict(GQ, GK, GV) of the existing single-slice call (attention_bwd_cases.backward_once)."""
    s = backward_slice(kind, name, D, Dv, dtype, scale, sq, skv)
    return BC.backward_once(plan_of(name), s["Q"], s["K"], s["V"], s["O"], s["GO"], s["LSE"], scale, dtype)


# ------------------------------------------------------- device helpers (GPU tests only) ----
def place_input(X, B, H, layout, dtype, shared=False):
    """X (Z, rows, W) fp32 on the host as a (B, H, rows, W) device view of `dtype` in `layout`,
    converted on the host. shared (K and V of "kv_shared"): one (B, 1, rows, W) tensor expanded over
    the heads; the slices of a batch must then be equal."""
    from gpu_util import to_device, torch_cuda
    torch = torch_cuda()
    Z, rows, W = X.shape
    assert Z == B * H
    X4 = np.asarray(X, np.float32).reshape(B, H, rows, W)
    if shared:
        assert all((X4[:, h].view(np.uint32) == X4[:, 0].view(np.uint32)).all() for h in range(H))
        return to_device(X4[:, :1], dtype).expand(B, H, rows, W)
    t = to_device(X4, dtype)
    if layout == "bmhd":
        t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        assert t.stride() == (rows * H * W, W, H * W, 1)
    elif layout == "padded":
        base = torch.full((B, H, rows, W + PAD), float("nan"), dtype=t.dtype, device="cuda")
        base[..., :W] = t
        t = base[..., :W]
    return t


def place_output(B, H, rows, W, layout):
    """(buffer, view): a (B, H, rows, W) fp32 view in `layout` of a buffer holding FILL_BITS, with
    GUARD more elements behind the last one."""
    from gpu_util import torch_cuda
    torch = torch_cuda()
    row = W + PAD if layout == "padded" else W
    n = B * H * rows * row
    buf = torch.full((n + GUARD,), FILL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    if layout == "bmhd":
        return buf, buf[:n].view(B, rows, H, W).permute(0, 2, 1, 3)
    return buf, buf[:n].view(B, H, rows, row)[..., :W]


def read_output(buf, view, what, written=True):
    """(Z, rows, W) numpy fp32 of an output after the launch. Every element of the view was written
    (or, written=False, none), and no element outside it (guard zone, row padding) changed."""
    from gpu_util import torch_cuda
    torch = torch_cuda()
    mask = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
    torch.as_strided(mask, view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(True)
    h, m = buf.cpu().numpy().view(np.uint32), mask.cpu().numpy()
    assert int(m.sum()) == view.numel(), "the output view overlaps itself"
    assert (h[~m] == FILL_BITS).all(), f"{what}: a store outside the output's elements (guard zone or row padding)"
    B, H, rows, W = view.shape
    Y = view.cpu().numpy().reshape(B * H, rows, W)
    if written:
        assert not (Y.view(np.uint32) == FILL_BITS).any(), f"{what}: an element was never written"
    else:
        assert (Y.view(np.uint32) == FILL_BITS).all(), f"{what}: written though it was not asked for"
    return Y


def _stream():
    from gpu_util import torch_cuda
    return torch_cuda().cuda.current_stream().cuda_stream


def out_layout(layout):
    return "bhmd" if layout == "kv_shared" else layout


def forward_inputs(slices, B, H, layout, dtype):
    """(dQ, dK, dV) device views of the stacked slices."""
    shared = layout == "kv_shared"
    return (place_input(stack(slices, "Q"), B, H, out_layout(layout), dtype),
            place_input(stack(slices, "K"), B, H, layout, dtype, shared),
            place_input(stack(slices, "V"), B, H, layout, dtype, shared))


def heads_forward_once(plan, slices, B, H, layout, scale, dtype=F32, lse=True, dev=None):
    """(O (Z, M, Dv), LSE (Z, M) or None) of one bsmr_attention_heads on the slices in `layout`."""
    from gpu_util import torch_cuda
    torch = torch_cuda()
    D, Dv = slices[0]["Q"].shape[1], slices[0]["V"].shape[1]
    dQ, dK, dV = dev or forward_inputs(slices, B, H, layout, dtype)
    bufO, vO = place_output(B, H, plan.M, Dv, out_layout(layout))
    bufL, vL = place_output(B, H, plan.M, 1, "bhmd")
    plan.attention_heads(B, H, dQ, dK, dV, D, Dv, vO, bufL.data_ptr() if lse else 0, scale, stream=_stream(), dtype=dtype)
    torch.cuda.synchronize()
    O = read_output(bufO, vO, "O")
    L = read_output(bufL, vL, "LSE", written=lse)
    return O, (L[:, :, 0] if lse else None)


def backward_inputs(slices, B, H, layout, dtype):
    """(dQ, dK, dV, dO, dGO, dLse): dLse dense (B, H, M)."""
    from gpu_util import to_device
    o = out_layout(layout)
    return forward_inputs(slices, B, H, layout, dtype) + (
        place_input(stack(slices, "O"), B, H, o, F32), place_input(stack(slices, "GO"), B, H, o, F32),
        to_device(stack(slices, "LSE").reshape(B, H, -1), F32))


def heads_backward_once(plan, slices, B, H, layout, scale, dtype=F32, want=OUTPUTS, dev=None):
    """dict(GQ, GK, GV) ((Z, rows, W) numpy fp32; None for an output not in `want`) of one
    bsmr_attention_backward_heads on the slices in `layout`."""
    from gpu_util import torch_cuda
    torch = torch_cuda()
    D, Dv = slices[0]["Q"].shape[1], slices[0]["V"].shape[1]
    d = dev or backward_inputs(slices, B, H, layout, dtype)
    shapes = dict(GQ=(plan.M, D), GK=(plan.N, D), GV=(plan.N, Dv))
    outs = {k: place_output(B, H, r, c, out_layout(layout)) for k, (r, c) in shapes.items()}
    arg = {k: (outs[k][1] if k in want else None) for k in OUTPUTS}
    plan.attention_backward_heads(B, H, d[0], d[1], d[2], d[3], d[4], d[5].data_ptr(), D, Dv, arg["GQ"], arg["GK"],
                                  arg["GV"], scale, stream=_stream(), dtype=dtype)
    torch.cuda.synchronize()
    out = {}
    for k in OUTPUTS:
        Y = read_output(*outs[k], k, written=k in want)
        out[k] = Y if k in want else None
    return out


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def assert_slices_equal(got, want_per_slice, what):
    """got (Z, rows, W) against a list of per-slice (rows, W) arrays, bit for bit."""
    for z, want in enumerate(want_per_slice):
        check_exact(got[z].reshape(np.asarray(want).shape[0], -1), np.asarray(want).reshape(len(want), -1),
                    f"{what} slice {z}")
