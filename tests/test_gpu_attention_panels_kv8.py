"""GPU: the panel attention forward over e4m3 K / V (bsmr_attention_panels_kv8)
on the six patterns of test_gpu_attention_panels.py: bit-exact selector data on the e4m3 grid; O and
LSE inside a derived bound of the float64 reference on the widened bytes and |O_kv8 - v_scale O_16|
inside the sum of the two paths' bounds; heads slices, NaN containment, refusals, capture; end to end.

Bounds (section 20). The converts are exact, so O carries section 18's bound (attention_bound +
panel_terms) plus u A for the rounded product (1 / l) v_scale, all times v_scale; LSE carries
lse_bound + 3 s u plus |m scale k_scale| u, the product scale k_scale being rounded once to fp32. The
16-bit launch gets that rounded product as its scale and rounds c from it, a relative u away from
the reference's scale: each of its weights moves by at most W_e (|d_e| + sum_i W_i |d_i|) u.
"""
import numpy as np
import pytest

import attention_cases as AC
import bsmr
from attention_cases import FILL_BITS, filled
from bsmr import BF16, F16, F32
from gpu_util import to_device, torch_cuda
from test_gpu_attention_panels import PATTERNS, lists_of, once, panel_terms, pattern, plan_of

pytestmark = pytest.mark.gpu
UNSUPPORTED, INVALID = 6, 1
U = 2.0 ** -24
FORMS = [pytest.param(dt, D, Dv, id=f"{AC.DTYPE_NAME[dt]}-{D}-{Dv}") for dt in (F16, BF16)
         for D, Dv in [(64, 128), (128, 64), (256, 256)]]


def quantized(K, V):
    """(K8, V8 on the device, their widened values on the host, k_scale, v_scale)."""
    import torch
    from bsmr.autograd import quantize_kv
    K8, V8, ks, vs = quantize_kv(torch.from_numpy(np.array(K, np.float32)), torch.from_numpy(np.array(V, np.float32)))
    return K8.cuda(), V8.cuda(), K8.float().numpy(), V8.float().numpy(), ks, vs


def once8(plan, dQ, dK8, dV8, scale, ks, vs, dtype):
    """(O, LSE) of one kv8 launch on device operands; both outputs start as FILL_BITS with a guard zone."""
    torch = torch_cuda()
    D, Dv = dQ.shape[1], dV8.shape[1]
    bufO, dO = filled(plan.M * Dv)
    bufL, dL = filled(plan.M)
    plan.attention_panels_kv8(dQ.data_ptr(), dK8.data_ptr(), dV8.data_ptr(), D, Dv, dO.data_ptr(), dL.data_ptr(), scale, ks,
                              vs, stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    hO, hL = bufO.cpu().numpy(), bufL.cpu().numpy()
    assert (hO[plan.M * Dv:].view(np.uint32) == FILL_BITS).all() and (hL[plan.M:].view(np.uint32) == FILL_BITS).all()
    assert not (hO[:plan.M * Dv].view(np.uint32) == FILL_BITS).any() and not (hL[:plan.M].view(np.uint32) == FILL_BITS).any()
    return hO[:plan.M * Dv].reshape(plan.M, Dv), hL[:plan.M]


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_selector_data_on_the_e4m3_grid_is_bit_exact(dtype, D, Dv, name):
    # rank = pi + 1 = 256 a + 16 b + c in K columns 0 .. 2, Q columns 256 q, 16 q, q: the score q rank
    # is three exact products summed exactly in any order
    pat, plan, q = pattern(name), plan_of(name), 128.0
    assert pat[1] < 4096
    for order, scale, ks, vs in (("random", 16.0, 1.0, 1.0), ("ascending", 2.0, 0.5, 4.0), ("descending", 4.0, 0.5, 1.0)):
        _, K, V, winner, pi, _ = AC.selector(pat, D, Dv, order, dtype)
        rank = pi + 1
        K *= 448.0  # signed junk under Q's zeros, one element at the top of the grid: the quantiser's scale is 1
        K[:, 0], K[:, 1], K[:, 2], K[0, 3] = rank // 256, rank // 16 % 16, rank % 16, 448.0
        dK8, dV8, Kw, Vw, k1, _ = quantized(K, 448.0 * V)
        assert k1 == 1.0 and (Kw[:, :3] == K[:, :3]).all()  # the rank columns survive the round trip
        Q = np.zeros((pat[0], D), np.float32)
        Q[:, :3] = 256 * q, 16 * q, q
        assert q * scale * ks * AC.LOG2E > 150  # the nearest loser's weight is 2^-150 or less: exactly 0 in fp32
        O, LSE = once8(plan, to_device(Q, dtype), dK8, dV8, scale, ks, vs, dtype)
        won = winner >= 0
        AC.check_exact(O, np.where(won[:, None], vs * Vw[np.maximum(winner, 0)], 0), f"O {name} {order}")
        wantL = np.where(won, scale * ks * q * rank[np.maximum(winner, 0)], -np.inf)
        assert (wantL.astype(np.float32) == wantL).all()
        AC.check_exact(LSE, wantL.astype(np.float32), f"LSE {name} {order}")


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_against_float64(dtype, D, Dv, name):
    pat, plan = pattern(name), plan_of(name)
    s = lists_of(name)[3]
    for kind, scale in (("narrow", 1.0), ("wide", 1.0), ("narrow", D ** -0.5), ("wide", D ** -0.5)):
        Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, kind, scale)
        dK8, dV8, Kw, Vw, ks, vs = quantized(K, V)
        scale = float(np.float32(scale))
        eff = scale * ks  # exact in double, as the library forms it
        dQ = to_device(Q, dtype)
        O, LSE = once8(plan, dQ, dK8, dV8, scale, ks, vs, dtype)
        O1, _ = once8(plan, dQ, dK8, dV8, scale, ks, 1.0, dtype)
        O16, _ = once(plan, Q, Kw, Vw, eff, dtype, dev=[dQ, to_device(Kw, dtype), to_device(Vw, dtype)])
        ref = AC.attention_ref(pat, Q, Kw, Vw, eff, dtype)
        A = AC._weighted(ref, ref["W"])
        b16 = AC.attention_bound(ref, opscale / ks) + panel_terms(ref, dtype, s)
        b8 = vs * (b16 + U * A)
        b16 = b16 + AC._weighted(ref, ref["W"] * (ref["d"] + ref["sd"]) * U)
        live = ref["lens"] > 0
        with np.errstate(invalid="ignore"):
            lb = AC.lse_bound(ref, opscale / ks) + 3 * s * U + np.where(live, np.abs(ref["m"] * eff), 0) * U
        ro = AC._ratio(np.abs(O - vs * ref["O"]), b8)
        rl = AC._ratio(np.abs(LSE[live] - ref["LSE"][live]), lb[live])
        rp = AC._ratio(np.abs(O.astype(np.float64) - vs * O16.astype(np.float64)), b8 + vs * b16)
        same = bool((O1.view(np.uint32) == O16.view(np.uint32)).all())
        print(f"RATIO attention_panels_kv8 {AC.DTYPE_NAME[dtype]} {D} {Dv} {name} {kind} {scale:.4f}: O {ro:.4f} LSE {rl:.4f} "
              f"vs panels16 {rp:.4f} bit-equal at v_scale 1: {same}")
        assert (O[~live] == 0).all() and (LSE[~live] == -np.inf).all()
        assert ro <= 1.0 and rl <= 1.0 and rp <= 1.0, (kind, scale, ro, rl, rp)


def _hub_inputs(D, Dv, dtype):
    pat = pattern("hub")
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "narrow", 0.125)
    return (pat, plan_of("hub"), to_device(Q, dtype)) + quantized(K, V)


def test_heads_slices_equal_the_single_slice_call():
    torch = torch_cuda()
    B, H, D, Dv, dtype = 2, 3, 64, 128, BF16  # hub has split panels: a scratch per slice
    pat, plan, _, dK8, dV8, _, _, ks, vs = _hub_inputs(D, Dv, dtype)
    M, N = pat[0], pat[1]
    Q = torch.from_numpy(AC.signed_data(B * M * H * D, 1)).to(torch.bfloat16).cuda().view(B, M, H, D).transpose(1, 2)
    per_batch = lambda X: X.view(torch.uint8).unsqueeze(0).repeat(B, 1, 1).view(X.dtype).unsqueeze(1)  # noqa: E731
    K8, V8 = per_batch(dK8).expand(B, H, N, D), per_batch(dV8).expand(B, H, N, Dv)  # one K8 / V8 per batch: head stride 0
    O = torch.full((B, M, H, Dv), float("nan"), device="cuda").transpose(1, 2)
    L = torch.full((B, H, M), float("nan"), device="cuda")
    plan.attention_panels_kv8_heads(B, H, Q, K8, V8, D, Dv, O, L.data_ptr(), 0.25, ks, vs,
                                    stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    for b in range(B):
        for h in range(H):
            o, l = once8(plan, Q[b, h].contiguous(), dK8, dV8, 0.25, ks, vs, dtype)
            assert np.array_equal(O[b, h].cpu().numpy().view(np.uint32), o.view(np.uint32)), (b, h)
            assert np.array_equal(L[b, h].cpu().numpy().view(np.uint32), l.view(np.uint32)), (b, h)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_nan_byte_stays_in_its_rows_and_panels(dtype):
    import torch
    pat, plan, dQ, dK8, dV8, _, _, ks, vs = _hub_inputs(64, 64, dtype)
    M, N, rp, ci = pat
    rows, cols, items, _ = lists_of("hub")
    clean = once8(plan, dQ, dK8, dV8, 0.125, ks, vs, dtype)
    j = int(ci[rp[5]])  # a column that a short row stores (the hub row stores it too)
    storing = np.zeros(M, bool)
    storing[AC.entry_rows(pat)[ci == j]] = True
    in_panel = np.zeros(M, bool)  # rows of the panels whose union holds j
    for row0, step0, nsteps, _ in items:
        if (cols[step0:step0 + nsteps] == j).any():
            in_panel[rows[row0:row0 + 16]] = True
    assert not in_panel.all(), "the pattern must have a panel that does not hold the column"
    for what, X, may in (("K", 0, storing), ("V", 1, in_panel)):
        ops = [dK8.clone(), dV8.clone()]
        ops[X].view(torch.uint8)[j, 3] = 0x7F
        O, LSE = once8(plan, dQ, *ops, 0.125, ks, vs, dtype)
        changed = (O.view(np.uint32) != clean[0].view(np.uint32)).any(axis=1)
        assert np.isnan(O[storing]).any(axis=1).all() and (changed == may).all(), what
        assert (np.isnan(LSE) == (storing if what == "K" else False)).all(), what
        assert (LSE.view(np.uint32) == clean[1].view(np.uint32))[~storing if what == "K" else slice(None)].all(), what


def test_refusals_and_capture():
    torch = torch_cuda()
    name, D, Dv = "split", 64, 64
    pat = pattern(name)
    plan = AC.make_plan(pat)  # a fresh plan: nothing prepared
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "narrow", 0.125)
    dQ = to_device(Q, F16)
    dK8, dV8, _, _, ks, vs = quantized(K, V)
    bufO, dO = filled(plan.M * Dv)
    bufL, dL = filled(plan.M)

    def status(s, D_=D, Dv_=Dv, dt=F16, ks_=ks, vs_=vs):
        with pytest.raises(bsmr.BsmrError) as ei:
            plan.attention_panels_kv8(dQ.data_ptr(), dK8.data_ptr(), dV8.data_ptr(), D_, Dv_, dO.data_ptr(), dL.data_ptr(),
                                      0.125, ks_, vs_, stream=s, dtype=dt)
        return ei.value.status

    s0 = torch.cuda.current_stream().cuda_stream
    assert status(s0, dt=F32) == UNSUPPORTED and status(s0, D_=32) == UNSUPPORTED and status(s0, Dv_=512) == UNSUPPORTED
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert status(s0, ks_=bad) == INVALID and status(s0, vs_=bad) == INVALID, bad
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        refused = status(side.cuda_stream)
    assert refused == bsmr.NOT_PREPARED and not plan.attention_panels_prepared(D, Dv)
    torch.cuda.synchronize()
    assert (bufO.cpu().numpy().view(np.uint32) == FILL_BITS).all() and (bufL.cpu().numpy().view(np.uint32) == FILL_BITS).all()
    plan.prepare_attention_panels(D, Dv)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # the first launch of the plan is the captured one
        plan.attention_panels_kv8(dQ.data_ptr(), dK8.data_ptr(), dV8.data_ptr(), D, Dv, dO.data_ptr(), dL.data_ptr(), 0.125, ks,
                                  vs, stream=side.cuda_stream, dtype=F16)
    eager = once8(plan_of(name), dQ, dK8, dV8, 0.125, ks, vs, F16)  # a lazily built plan
    for _ in range(3):
        dO.fill_(float("nan"))
        dL.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        AC.check_exact(dO.cpu().numpy().reshape(plan.M, Dv), eager[0], "replay O")
        AC.check_exact(dL.cpu().numpy(), eager[1], "replay LSE")


def test_attention_fused_kv8_against_dense_float64_attention():
    # tolerance: 8 x the error of the same dense attention computed in float16 on the CPU, against float64
    torch = torch_cuda()
    from bsmr import autograd
    from test_gpu_attention_fused_autograd import _dense_attention, _t
    pat = AC.pattern("zipf_shuffled")
    plan = AC.make_plan(pat)
    M, N, D = pat[0], pat[1], 64
    Q, K, V = (AC.signed_data(r * D, 81 + i).reshape(r, D) for i, r in enumerate((M, N, N)))
    tQ = _t(torch, Q, torch.float16, grad=False)
    K8, V8, Kw, Vw, ks, vs = quantized(K, V)
    args = (pat, tQ.float().cpu().numpy(), Kw * np.float32(ks), Vw * np.float32(vs), np.zeros((M, D), np.float32), D ** -0.5)
    ref, cpu = _dense_attention(*args, np.float64)[0], _dense_attention(*args, np.float16)[0]
    O, lse = autograd.attention_fused_kv8(plan, tQ, K8, V8, ks, vs, return_lse=True)
    torch.cuda.synchronize()
    assert O.shape == (M, D) and lse.shape == (M,) and not O.requires_grad and plan.attention_panels_stats()["items"] > 0
    top = np.abs(ref).max()
    cpu_err = np.abs(cpu.astype(np.float64) - ref).max() / top
    gpu_err = np.abs(O.cpu().numpy().astype(np.float64) - ref).max() / top
    print(f"ATTENTION_PANELS_KV8 f16 O: float16 CPU error {cpu_err:.3e}, GPU error {gpu_err:.3e}")
    assert 0 < cpu_err and gpu_err <= 8 * cpu_err
    with pytest.raises(ValueError, match="no backward"):
        autograd.attention_fused_kv8(plan, tQ.clone().requires_grad_(True), K8, V8, ks, vs)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        autograd.attention_fused_kv8(plan, tQ, K8.to(torch.float16), V8, ks, vs)
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        autograd.attention_fused_kv8(plan, tQ.float(), K8, V8, ks, vs)
