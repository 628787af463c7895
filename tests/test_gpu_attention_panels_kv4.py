"""GPU: the panel attention forward over an MXFP4 K / V cache (bsmr_attention_panels_kv4, DESIGN.md
section 25) on the six patterns of test_gpu_attention_panels.py. quantize_kv_mx4 keeps every block
exponent in [-12, 0], where the convert is exact in fp16 and bf16, so the bounds are section 20's
(test_gpu_attention_panels_kv8.py's docstring) with the records' values for the widened bytes."""
import numpy as np
import pytest

import attention_cases as AC
import bsmr
from attention_cases import FILL_BITS, filled
from bsmr import BF16, F16, F32, mx4_record_bytes
from gpu_util import to_device, torch_cuda
from test_gpu_attention_panels import PATTERNS, lists_of, once, panel_terms, pattern, plan_of

pytestmark = pytest.mark.gpu
UNSUPPORTED, INVALID = 6, 1
U = 2.0 ** -24
GRID = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6], np.float32)
FORMS = [pytest.param(dt, D, Dv, id=f"{AC.DTYPE_NAME[dt]}-{D}-{Dv}") for dt in (F16, BF16)
         for D, Dv in [(128, 128), (128, 256), (256, 128)]]


def quantized(K, V):
    """(K4, V4 on the device, the records' values on the host, k_scale, v_scale)."""
    import torch
    from bsmr.autograd import dequantize_mx4, quantize_kv_mx4
    K4, V4, ks, vs = quantize_kv_mx4(torch.from_numpy(np.array(K, np.float32)), torch.from_numpy(np.array(V, np.float32)))
    values = [dequantize_mx4(X4, X.shape[-1], torch.float32).numpy() for X4, X in ((K4, K), (V4, V))]
    return K4.cuda(), V4.cuda(), values[0], values[1], ks, vs


def once4(plan, dQ, dK4, dV4, Dv, scale, ks, vs, dtype):
    """(O, LSE) of one kv4 launch on device operands; both outputs start as FILL_BITS with a guard zone."""
    torch = torch_cuda()
    bufO, dO = filled(plan.M * Dv)
    bufL, dL = filled(plan.M)
    plan.attention_panels_kv4(dQ.data_ptr(), dK4.data_ptr(), dV4.data_ptr(), dQ.shape[1], Dv, dO.data_ptr(), dL.data_ptr(),
                              scale, ks, vs, stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    hO, hL = bufO.cpu().numpy(), bufL.cpu().numpy()
    assert (hO[plan.M * Dv:].view(np.uint32) == FILL_BITS).all() and (hL[plan.M:].view(np.uint32) == FILL_BITS).all()
    assert not (hO[:plan.M * Dv].view(np.uint32) == FILL_BITS).any() and not (hL[:plan.M].view(np.uint32) == FILL_BITS).any()
    return hO[:plan.M * Dv].reshape(plan.M, Dv), hL[:plan.M]


def on_grid(rows, W, period, seed):
    """Grid data: random e2m1 codes times 2^-(b % period) in block b, the block's last element
    -6 2^-(b % period) so that the quantiser finds that exponent again (block 0: the tensor's amax 6)."""
    X = GRID[np.random.default_rng(seed).integers(0, 16, (rows, W))]
    X[:, 31::32] = -6.0
    return X * np.exp2(-(np.arange(W) // 32 % period)).astype(np.float32)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_selector_data_on_the_e2m1_grid_is_bit_exact(dtype, D, Dv, name):
    # rank = pi + 1 in base 4: digit t sits at K element pos[t] as the e2m1 value d_t times its block's
    # 2^-(b % 4), and Q there is q 4^t 2^(b % 4): the score q rank is six exact products summed exactly
    # in any order. The positions cover six blocks (four at D = 128), all four words of a chunk, low
    # and high nibbles; everything else of K is signed grid junk under Q's zeros
    pat, plan, q = pattern(name), plan_of(name), 16.0
    assert pat[1] < 4096
    pos = (np.arange(6) * 37 + 3) % D
    assert (pos % 32 != 31).all() and len(set(pos // 32)) == min(6, D // 32)
    for order, scale, ks, vs in (("random", 16.0, 1.0, 1.0), ("ascending", 32.0, 0.5, 4.0), ("descending", 16.0, 0.5, 1.0)):
        _, _, _, winner, pi, _ = AC.selector(pat, D, Dv, order, dtype)
        rank = pi + 1
        K, V = on_grid(pat[1], D, 4, 21), on_grid(pat[1], Dv, 3, 22)
        Q = np.zeros((pat[0], D), np.float32)
        for t, c in enumerate(pos):
            K[:, c] = (rank >> 2 * t & 3) * 2.0 ** -(c // 32 % 4)
            Q[:, c] = q * 4.0 ** t * 2.0 ** (c // 32 % 4)
        dK4, dV4, Kw, Vw, k1, v1 = quantized(K, V)
        assert k1 == 1.0 and v1 == 1.0 and (Kw == K).all() and (Vw == V).all()  # the data survives the round trip
        assert q * scale * ks * AC.LOG2E > 150  # the nearest loser's weight is 2^-150 or less: exactly 0 in fp32
        O, LSE = once4(plan, to_device(Q, dtype), dK4, dV4, Dv, scale, ks, vs, dtype)
        won = winner >= 0
        AC.check_exact(O, np.where(won[:, None], vs * Vw[np.maximum(winner, 0)], 0), f"O {name} {order}")
        wantL = np.where(won, scale * ks * q * rank[np.maximum(winner, 0)], -np.inf)
        assert (wantL.astype(np.float32) == wantL).all()
        AC.check_exact(LSE, wantL.astype(np.float32), f"LSE {name} {order}")


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_against_float64_and_the_16_bit_panel_forward(dtype, D, Dv, name):
    pat, plan = pattern(name), plan_of(name)
    s = lists_of(name)[3]
    for kind, scale in (("narrow", 1.0), ("wide", 1.0), ("narrow", D ** -0.5), ("wide", D ** -0.5)):
        Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, kind, scale)
        dK4, dV4, Kw, Vw, ks, vs = quantized(K, V)
        scale = float(np.float32(scale))
        eff = scale * ks  # exact in double, as the library forms it
        dQ = to_device(Q, dtype)
        O, LSE = once4(plan, dQ, dK4, dV4, Dv, scale, ks, vs, dtype)
        O16, _ = once(plan, Q, Kw, Vw, eff, dtype, dev=[dQ, to_device(Kw, dtype), to_device(Vw, dtype)])
        ref = AC.attention_ref(pat, Q, Kw, Vw, eff, dtype)
        A = AC._weighted(ref, ref["W"])
        b16 = AC.attention_bound(ref, opscale / ks) + panel_terms(ref, dtype, s)
        b4 = vs * (b16 + U * A)
        b16 = b16 + AC._weighted(ref, ref["W"] * (ref["d"] + ref["sd"]) * U)
        live = ref["lens"] > 0
        with np.errstate(invalid="ignore"):
            lb = AC.lse_bound(ref, opscale / ks) + 3 * s * U + np.where(live, np.abs(ref["m"] * eff), 0) * U
        ro = AC._ratio(np.abs(O - vs * ref["O"]), b4)
        rl = AC._ratio(np.abs(LSE[live] - ref["LSE"][live]), lb[live])
        rp = AC._ratio(np.abs(O.astype(np.float64) - vs * O16.astype(np.float64)), b4 + vs * b16)
        print(f"RATIO attention_panels_kv4 {AC.DTYPE_NAME[dtype]} {D} {Dv} {name} {kind} {scale:.4f}: O {ro:.4f} LSE {rl:.4f} "
              f"vs panels16 {rp:.4f}")
        assert (O[~live] == 0).all() and (LSE[~live] == -np.inf).all()
        assert ro <= 1.0 and rl <= 1.0 and rp <= 1.0, (kind, scale, ro, rl, rp)


def _hub_inputs(D, Dv, dtype):
    pat = pattern("hub")
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "narrow", 0.125)
    return (pat, plan_of("hub"), to_device(Q, dtype)) + quantized(K, V)


def test_heads_slices_equal_the_single_slice_call():
    torch = torch_cuda()
    B, H, D, Dv, dtype = 2, 3, 128, 256, BF16  # hub has split panels: a scratch per slice
    pat, plan, _, dK4, dV4, _, _, ks, vs = _hub_inputs(D, Dv, dtype)
    M, N = pat[0], pat[1]
    Q = torch.from_numpy(AC.signed_data(B * M * H * D, 1)).to(torch.bfloat16).cuda().view(B, M, H, D).transpose(1, 2)
    K4 = dK4.expand(B, H, N, mx4_record_bytes(D))  # one K4 for every slice: batch and head stride 0
    V4 = dV4.repeat(B, H, 1, 1)                    # a V4 of its own per slice
    O = torch.full((B, M, H, Dv), float("nan"), device="cuda").transpose(1, 2)
    L = torch.full((B, H, M), float("nan"), device="cuda")
    plan.attention_panels_kv4_heads(B, H, Q, K4, V4, D, Dv, O, L.data_ptr(), 0.25, ks, vs,
                                    stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    for b in range(B):
        for h in range(H):
            o, l = once4(plan, Q[b, h].contiguous(), dK4, dV4, Dv, 0.25, ks, vs, dtype)
            assert np.array_equal(O[b, h].cpu().numpy().view(np.uint32), o.view(np.uint32)), (b, h)
            assert np.array_equal(L[b, h].cpu().numpy().view(np.uint32), l.view(np.uint32)), (b, h)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_nan_scale_byte_stays_in_its_rows_and_panels(dtype):
    D = Dv = 128
    pat, plan, dQ, dK4, dV4, _, _, ks, vs = _hub_inputs(D, Dv, dtype)
    M, N, rp, ci = pat
    rows, cols, items, _ = lists_of("hub")
    clean = once4(plan, dQ, dK4, dV4, Dv, 0.125, ks, vs, dtype)
    j = int(ci[rp[5]])  # a column that a short row stores (the hub row stores it too)
    storing = np.zeros(M, bool)
    storing[AC.entry_rows(pat)[ci == j]] = True
    in_panel = np.zeros(M, bool)  # rows of the panels whose union holds j
    for row0, step0, nsteps, _ in items:
        if (cols[step0:step0 + nsteps] == j).any():
            in_panel[rows[row0:row0 + 16]] = True
    assert not in_panel.all(), "the pattern must have a panel that does not hold the column"
    for what, X, may in (("K", 0, storing), ("V", 1, in_panel)):
        ops = [dK4.clone(), dV4.clone()]
        ops[X][j, D // 2 + 2] = 0xFF  # the scale byte of block 2
        O, LSE = once4(plan, dQ, *ops, Dv, 0.125, ks, vs, dtype)
        changed = (O.view(np.uint32) != clean[0].view(np.uint32)).any(axis=1)
        assert np.isnan(O[storing]).any(axis=1).all() and (changed == may).all(), what
        assert (np.isnan(LSE) == (storing if what == "K" else False)).all(), what
        assert (LSE.view(np.uint32) == clean[1].view(np.uint32))[~storing if what == "K" else slice(None)].all(), what
    Qn = dQ.clone()
    Qn[5, 70] = float("nan")  # a NaN in Q stays in its row (row 5 stores j)
    O, LSE = once4(plan, Qn, dK4, dV4, Dv, 0.125, ks, vs, dtype)
    hit = np.arange(M) == 5
    assert (np.isnan(O).any(axis=1) == hit).all() and (np.isnan(LSE) == hit).all()
    assert (O[~hit].view(np.uint32) == clean[0][~hit].view(np.uint32)).all()


def test_refusals_and_capture():
    torch = torch_cuda()
    name, D, Dv = "split", 128, 128
    pat = pattern(name)
    plan = AC.make_plan(pat)  # a fresh plan: nothing prepared
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "narrow", 0.125)
    dQ = to_device(Q, F16)
    dK4, dV4, _, _, ks, vs = quantized(K, V)
    assert vs != 1.0  # the split panel's reduce applies it
    bufO, dO = filled(plan.M * Dv)
    bufL, dL = filled(plan.M)

    def status(s, D_=D, Dv_=Dv, dt=F16, ks_=ks, vs_=vs, k_off=0):
        with pytest.raises(bsmr.BsmrError) as ei:
            plan.attention_panels_kv4(dQ.data_ptr(), dK4.data_ptr() + k_off, dV4.data_ptr(), D_, Dv_, dO.data_ptr(),
                                      dL.data_ptr(), 0.125, ks_, vs_, stream=s, dtype=dt)
        return ei.value.status

    s0 = torch.cuda.current_stream().cuda_stream
    assert status(s0, dt=F32) == UNSUPPORTED
    for bad in (32, 64, 512):
        assert status(s0, D_=bad) == UNSUPPORTED and status(s0, Dv_=bad) == UNSUPPORTED, bad
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert status(s0, ks_=bad) == INVALID and status(s0, vs_=bad) == INVALID, bad
    assert status(s0, k_off=8) == INVALID
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        refused = status(side.cuda_stream)
    assert refused == bsmr.NOT_PREPARED and not plan.attention_panels_prepared(D, Dv)
    torch.cuda.synchronize()
    assert (bufO.cpu().numpy().view(np.uint32) == FILL_BITS).all() and (bufL.cpu().numpy().view(np.uint32) == FILL_BITS).all()
    plan.prepare_attention_panels(D, Dv)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # the first launch of the plan is the captured one
        plan.attention_panels_kv4(dQ.data_ptr(), dK4.data_ptr(), dV4.data_ptr(), D, Dv, dO.data_ptr(), dL.data_ptr(), 0.125, ks,
                                  vs, stream=side.cuda_stream, dtype=F16)
    eager = once4(plan_of(name), dQ, dK4, dV4, Dv, 0.125, ks, vs, F16)  # a lazily built plan
    for _ in range(3):
        dO.fill_(float("nan"))
        dL.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        AC.check_exact(dO.cpu().numpy().reshape(plan.M, Dv), eager[0], "replay O")
        AC.check_exact(dL.cpu().numpy(), eager[1], "replay LSE")


def test_attention_fused_kv4_against_dense_float64_attention():
    # tolerance: 8 x the error of the same dense attention computed in float16 on the CPU, against float64
    torch = torch_cuda()
    from bsmr import autograd
    from test_gpu_attention_fused_autograd import _dense_attention, _t
    pat = AC.pattern("zipf_shuffled")
    plan = AC.make_plan(pat)
    M, N, D = pat[0], pat[1], 128
    Q, K, V = (AC.signed_data(r * D, 81 + i).reshape(r, D) for i, r in enumerate((M, N, N)))
    tQ = _t(torch, Q, torch.float16, grad=False)
    K4, V4, Kw, Vw, ks, vs = quantized(K, V)
    args = (pat, tQ.float().cpu().numpy(), Kw * np.float32(ks), Vw * np.float32(vs), np.zeros((M, D), np.float32), D ** -0.5)
    ref, cpu = _dense_attention(*args, np.float64)[0], _dense_attention(*args, np.float16)[0]
    O, lse = autograd.attention_fused_kv4(plan, tQ, K4, V4, ks, vs, return_lse=True)
    torch.cuda.synchronize()
    assert O.shape == (M, D) and lse.shape == (M,) and not O.requires_grad and plan.attention_panels_stats()["items"] > 0
    top = np.abs(ref).max()
    cpu_err = np.abs(cpu.astype(np.float64) - ref).max() / top
    gpu_err = np.abs(O.cpu().numpy().astype(np.float64) - ref).max() / top
    print(f"ATTENTION_PANELS_KV4 f16 O: float16 CPU error {cpu_err:.3e}, GPU error {gpu_err:.3e}")
    assert 0 < cpu_err and gpu_err <= 8 * cpu_err
    for match, call in (("no backward", lambda: autograd.attention_fused_kv4(plan, tQ.clone().requires_grad_(True), K4, V4, ks, vs)),
                        ("torch.uint8", lambda: autograd.attention_fused_kv4(plan, tQ, K4.to(torch.int8), V4, ks, vs)),
                        ("float16 or bfloat16", lambda: autograd.attention_fused_kv4(plan, tQ.float(), K4, V4, ks, vs)),
                        ("K4 must be", lambda: autograd.attention_fused_kv4(plan, tQ, K4[:-1], V4, ks, vs)),
                        ("one of 128, 256", lambda: autograd.attention_fused_kv4(plan, tQ[:, :64], K4[:, :48], V4, ks, vs)),
                        ("finite and > 0", lambda: autograd.attention_fused_kv4(plan, tQ, K4, V4, 0.0, vs))):
        with pytest.raises(ValueError, match=match):
            call()
