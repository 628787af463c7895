"""GPU: bsmr.autograd.attention_fused_heads: one Plan.attention_heads call forward and one
Plan.attention_backward_heads call backward over (B, H) slices of one pattern. zipf_shuffled, D = 32,
Dv = 48, fp32 and fp16, B = 2, H = 2, with Q, K and V taken as transposed views of (B, M, H D)
projections, passed as they are.

* O and each gradient are bit-equal per slice to attention_fused(..., backward="fused") on
  contiguous copies; O is dense in Q's dimension order, so O.transpose(1, 2).reshape(B, M, H Dv) is a
  view; LSE is (B, H, M), non-differentiable; the forward saves Q, K, V, O and LSE;
* end to end against the dense float64 masked attention per slice by the project's rule
  (tests/test_gpu_attention_bwd_autograd.py): per tensor 8 x the error of the same dense computation
  in float32 on the CPU, relative to max |ref|; at fp16 a gradient is held to 8 x the error of the
  float32 CPU gradient cast to fp16 once;
* K and V expanded over the heads (head stride 0, no copy): torch sums the head gradients, which is
  held to the float64 reference by the same rule, not to bits;
* needs_input_grad subsets give the full call's gradients bit for bit; (H, M, D) operands without a
  batch work alike;
* the ValueErrors are raised before any launch or build;
* memory, on the dense 512 x 512 pattern at D = Dv = 16 with Z = 4: torch's peak grows during
  .backward() by less than Z nnz 4 bytes (the gradients plus at most one contiguous copy of GO).
"""
import functools

import numpy as np
import pytest

import attention_cases as AC
from bsmr import F16, F32
from gpu_util import half_values, torch_cuda
from sddmm_cases import signed_data
from test_gpu_attention_fused_autograd import _dense_attention, _same_bits

pytestmark = pytest.mark.gpu
NAME = "zipf_shuffled"
B, H, D, DV = 2, 2, 32, 48


@functools.lru_cache(maxsize=None)
def _plan():
    return AC.make_plan(AC.pattern(NAME))


def _projections(seed, dtype, kv_heads=H):
    """Host (B, M, H D), (B, N, kv_heads D), (B, N, kv_heads Dv) projections and dO (B, M, H Dv), as
    every path sees them (rounded to fp16 first at fp16)."""
    pat = AC.pattern(NAME)
    M, N = pat[0], pat[1]
    xq = signed_data(B * M * H * D, seed).reshape(B, M, H * D)
    xk = signed_data(B * N * kv_heads * D, seed + 1).reshape(B, N, kv_heads * D)
    xv = signed_data(B * N * kv_heads * DV, seed + 2).reshape(B, N, kv_heads * DV)
    dO = signed_data(B * M * H * DV, seed + 3).reshape(B, M, H * DV)
    if dtype != F32:
        xq, xk, xv = (half_values(X, dtype) for X in (xq, xk, xv))
    return xq, xk, xv, dO


def _leaf(torch, x, tdt, grad=True):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(tdt).cuda().requires_grad_(grad)


def _heads_view(t, heads, W):
    """(B, rows, heads W) -> (B, heads, rows, W), a view."""
    return t.view(t.shape[0], t.shape[1], heads, W).transpose(1, 2)


def _np_slice(x, h, W):
    return x[:, h * W:(h + 1) * W]


def _check_rule(name, dtype, got, ref, f32, is_grad, failures):
    top = np.abs(ref).max()
    cpu = half_values(f32, dtype) if (dtype != F32 and is_grad) else f32
    cpu_err = np.abs(cpu.astype(np.float64) - ref).max() / top
    gpu_err = np.abs(got.astype(np.float64) - ref).max() / top
    print(f"ATTENTION_HEADS {AC.DTYPE_NAME[dtype]} {name}: float32 CPU error {cpu_err:.3e}, GPU error {gpu_err:.3e}, "
          f"tolerance {8 * cpu_err:.3e}")
    assert cpu_err > 0
    if not gpu_err <= 8 * cpu_err:
        failures.append((name, gpu_err, 8 * cpu_err))


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_transposed_views_per_slice_bits_and_float64(dtype):
    torch = torch_cuda()
    from bsmr import autograd
    pat, plan = AC.pattern(NAME), _plan()
    M, N = pat[0], pat[1]
    tdt = torch.float32 if dtype == F32 else torch.float16
    scale = D ** -0.5
    xq, xk, xv, dO = _projections(61, dtype)
    tq, tk, tv = (_leaf(torch, X, tdt) for X in (xq, xk, xv))
    Q, K, V = _heads_view(tq, H, D), _heads_view(tk, H, D), _heads_view(tv, H, DV)
    assert not Q.is_contiguous() and Q.data_ptr() == tq.data_ptr()
    O, LSE = autograd.attention_fused_heads(plan, Q, K, V, return_lse=True)
    assert O.dtype == torch.float32 and tuple(O.shape) == (B, H, M, DV) and O.requires_grad
    assert tuple(LSE.shape) == (B, H, M) and not LSE.requires_grad
    flat = O.transpose(1, 2).reshape(B, M, H * DV)
    assert flat.data_ptr() == O.data_ptr() and flat.is_contiguous(), "O is not dense in Q's dimension order"
    saved = O.grad_fn.saved_tensors
    assert len(saved) == 5 and not any(plan.nnz in t.shape or t.numel() in (plan.nnz, B * H * plan.nnz) for t in saved)
    assert [t.data_ptr() for t in saved[:3]] == [tq.data_ptr(), tk.data_ptr(), tv.data_ptr()], "an operand was copied"
    tdO = torch.from_numpy(dO).cuda()
    flat.backward(tdO, retain_graph=True)
    torch.cuda.synchronize()
    grads = [t.grad.clone() for t in (tq, tk, tv)]
    assert all(g.dtype == tdt and g.shape == t.shape for g, t in zip(grads, (tq, tk, tv)))
    hO, hL = O.detach().cpu().numpy(), LSE.cpu().numpy()
    hg = [g.float().cpu().numpy() for g in grads]
    failures = []
    for b in range(B):
        for h in range(H):
            sQ, sK, sV, sdO = (_np_slice(xq[b], h, D), _np_slice(xk[b], h, D), _np_slice(xv[b], h, DV),
                               _np_slice(dO[b], h, DV))
            # bit for bit: the single-slice function on contiguous copies
            ts = [_leaf(torch, X, tdt) for X in (sQ, sK, sV)]
            O1, L1 = autograd.attention_fused(plan, *ts, scale=scale, return_lse=True, backward="fused")
            O1.backward(torch.from_numpy(np.ascontiguousarray(sdO)).cuda())
            torch.cuda.synchronize()
            assert _same_bits(O[b, h].detach(), O1.detach()), f"O of slice ({b}, {h})"
            assert _same_bits(LSE[b, h], L1), f"LSE of slice ({b}, {h})"
            for name, g, t, W in zip(("dQ", "dK", "dV"), grads, ts, (D, D, DV)):
                assert _same_bits(g[b][:, h * W:(h + 1) * W], t.grad), f"{name} of slice ({b}, {h})"
            # the float64 rule
            ref = _dense_attention(pat, sQ, sK, sV, sdO, scale, np.float64)
            f32 = _dense_attention(pat, sQ, sK, sV, sdO, scale, np.float32)
            got = (hO[b, h], _np_slice(hg[0][b], h, D), _np_slice(hg[1][b], h, D), _np_slice(hg[2][b], h, DV))
            for i, name in enumerate(("O", "dQ", "dK", "dV")):
                _check_rule(f"slice ({b}, {h}) {name}", dtype, got[i], ref[i], f32[i], i > 0, failures)
    assert not failures, failures
    assert np.isfinite(hL[:, :, AC.row_lengths(pat) > 0]).all()
    # only some inputs need a gradient: the same bits as the full call
    for need in ((True, False, False), (False, False, True), (False, True, True)):
        ts = [_leaf(torch, X, tdt, grad=n) for X, n in zip((xq, xk, xv), need)]
        O2 = autograd.attention_fused_heads(plan, _heads_view(ts[0], H, D), _heads_view(ts[1], H, D),
                                            _heads_view(ts[2], H, DV))
        O2.transpose(1, 2).reshape(B, M, H * DV).backward(tdO)
        torch.cuda.synchronize()
        for name, t, n, g in zip(("dQ", "dK", "dV"), ts, need, grads):
            assert (t.grad is None) == (not n), (need, name)
            assert not n or _same_bits(t.grad, g), f"needs_input_grad {need}: {name} differs from the full call"
    # (H, M, D) operands without a batch: batch 1 of the call above
    ts = [_leaf(torch, X[1], tdt) for X in (xq, xk, xv)]
    v3 = [t.view(t.shape[0], H, W).transpose(0, 1) for t, W in zip(ts, (D, D, DV))]
    O3, L3 = autograd.attention_fused_heads(plan, *v3, return_lse=True)
    assert tuple(O3.shape) == (H, M, DV) and tuple(L3.shape) == (H, M)
    O3.transpose(0, 1).reshape(M, H * DV).backward(tdO[1])
    torch.cuda.synchronize()
    assert _same_bits(O3.detach(), O[1].detach()) and _same_bits(L3, LSE[1])
    for name, t, g in zip(("dQ", "dK", "dV"), ts, grads):
        assert _same_bits(t.grad, g[1]), f"{name} without a batch dimension"


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_expanded_k_and_v_sum_their_head_gradients(dtype):
    torch = torch_cuda()
    from bsmr import autograd
    pat, plan = AC.pattern(NAME), _plan()
    M, N = pat[0], pat[1]
    tdt = torch.float32 if dtype == F32 else torch.float16
    scale = D ** -0.5
    xq, xk, xv, dO = _projections(71, dtype, kv_heads=1)
    tq, tk, tv = (_leaf(torch, X, tdt) for X in (xq, xk, xv))
    K, V = tk.view(B, 1, N, D).expand(B, H, N, D), tv.view(B, 1, N, DV).expand(B, H, N, DV)
    assert K.stride(1) == 0 and K.data_ptr() == tk.data_ptr()
    O = autograd.attention_fused_heads(plan, _heads_view(tq, H, D), K, V)
    saved = O.grad_fn.saved_tensors
    assert [t.data_ptr() for t in saved[:3]] == [tq.data_ptr(), tk.data_ptr(), tv.data_ptr()], "an operand was copied"
    O.transpose(1, 2).reshape(B, M, H * DV).backward(torch.from_numpy(dO).cuda())
    torch.cuda.synchronize()
    assert tk.grad.shape == tk.shape and tv.grad.shape == tv.shape and tk.grad.dtype == tdt
    hO = O.detach().cpu().numpy()
    gq, gk, gv = (t.grad.float().cpu().numpy() for t in (tq, tk, tv))
    failures = []
    for b in range(B):
        refs, f32s = [], []
        for h in range(H):
            args = (pat, _np_slice(xq[b], h, D), xk[b], xv[b], _np_slice(dO[b], h, DV), scale)
            refs.append(_dense_attention(*args, np.float64))
            f32s.append(_dense_attention(*args, np.float32))
            _check_rule(f"expanded ({b}, {h}) O", dtype, hO[b, h], refs[h][0], f32s[h][0], False, failures)
            _check_rule(f"expanded ({b}, {h}) dQ", dtype, _np_slice(gq[b], h, D), refs[h][1], f32s[h][1], True, failures)
        for i, name, g in ((2, "dK", gk), (3, "dV", gv)):
            ref = sum(r[i] for r in refs)
            f32 = functools.reduce(lambda x, y: (x + y).astype(np.float32), [f[i] for f in f32s])
            _check_rule(f"expanded batch {b} {name} summed over heads", dtype, g[b], ref, f32, True, failures)
    assert not failures, failures


def test_value_errors_before_any_launch_or_build():
    torch = torch_cuda()
    from bsmr import autograd
    pat = AC.pattern("empty")
    M, N = pat[0], pat[1]
    plan = AC.make_plan(pat)
    z = functools.partial(torch.zeros, dtype=torch.float32, device="cuda")
    good = lambda: [z((H, M, 32)), z((H, N, 32)), z((H, N, 48))]  # noqa: E731

    def bad(i, t, match, a=None):
        a = a or good()
        a[i] = t
        with pytest.raises(ValueError, match=match):
            autograd.attention_fused_heads(plan, *a)

    bad(0, z((M, 32)), "Q must be")
    bad(0, z((H, M + 1, 32)), "Q must be")
    bad(1, z((H + 1, N, 32)), "K must be")
    bad(2, z((1, H, N, 48)), "V must be")
    bad(1, z((H, N, 32)).half(), "share one dtype")
    bad(0, z((H, M, 32)).cpu(), "device tensor")
    bad(0, z((H, M, 24)), "multiple of 16", [None, z((H, N, 24)), z((H, N, 48))])
    bad(2, z((H, N, 40)), "multiple of 16|of 16")
    bad(0, z((H, 32, M)).transpose(1, 2), "contiguous last dimension")
    bad(0, z((H, M, 34))[..., :32], "row stride")       # 136-byte rows
    bad(1, z((H, N, 36))[..., 1:33], "aligned")          # 4 bytes off
    bad(2, z((H, N, 48))[:, :1].expand(H, N, 48), "row stride")  # a row stride of 0
    with pytest.raises(ValueError, match="scale"):
        autograd.attention_fused_heads(plan, *good(), scale=0.0)
    with pytest.raises(ValueError, match="Q must be"):
        autograd.attention_fused_heads(plan, None, *good()[1:])
    assert not plan.attention_heads_prepared(32, 48, 1) and not plan.attention_backward_heads_prepared(32, 48, 1)
    assert not plan.attention_prepared(32, 48) and not plan.attention_backward_prepared(32, 48)
    # the good call itself passes
    O = autograd.attention_fused_heads(plan, *good())
    assert tuple(O.shape) == (H, M, 48) and plan.attention_heads_prepared(32, 48, H)


def test_backward_allocates_nothing_of_nnz_size():
    torch = torch_cuda()
    from bsmr import autograd
    n, d, Z = 512, 16, B * H
    rp = (np.arange(n + 1) * n).astype(np.uint32)
    ci = np.tile(np.arange(n, dtype=np.uint32), n)
    plan = AC.make_plan((n, n, rp, ci))
    nnz_bytes = plan.nnz * 4
    assert nnz_bytes == 1 << 20
    X = [signed_data(B * n * H * d, 7 + i).reshape(B, n, H * d) for i in range(4)]
    for attempt in range(2):  # the first pass builds the plan's lists and warms the allocator
        ts = [_leaf(torch, x, torch.float32) for x in X[:3]]
        O = autograd.attention_fused_heads(plan, *(_heads_view(t, H, d) for t in ts))
        out = O.transpose(1, 2).reshape(B, n, H * d)
        tdO = torch.from_numpy(X[3]).cuda()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out.backward(tdO)
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - before
        del O, out, ts
    operand = B * n * H * d * 4
    print(f"ATTENTION_HEADS memory: the backward grows torch's peak by {grew} bytes (Z nnz x 4 = {Z * nnz_bytes}, "
          f"one dense operand {operand})")
    assert grew < Z * nnz_bytes, grew
