"""GPU: bsmr.autograd.attention_fused, the differentiable sparse attention whose forward is the one
fused launch (Plan.attention) and whose backward recomputes the scores and weights. zipf_shuffled,
D = 32, Dv = 48, fp32 and fp16.

* dQ, dK and dV equal those of bsmr.autograd.attention bit for bit (the backward does not read O);
* O is inside attention_bound of the float64 reference; LSE is returned with requires_grad False
  and inside lse_bound;
* the forward keeps no tensor of nnz elements: O.grad_fn.saved_tensors are Q, K and V;
* two backward passes accumulate;
* end to end against the float64 dense masked attention on the CPU: per tensor 8 x the error of
  the same dense computation in float32 on the CPU, both errors printed (the rule of
  tests/test_gpu_attention_autograd.py);
* ValueError before any launch for what attention refuses, a V of another dtype and rows over the
  byte cap.
"""
import functools

import numpy as np
import pytest

import attention_cases as AC
from bsmr import F16, F32
from gpu_util import torch_cuda
from sddmm_cases import signed_data

pytestmark = pytest.mark.gpu
NAME = "zipf_shuffled"
D, DV = 32, 48


@functools.lru_cache(maxsize=None)
def _plan():
    return AC.make_plan(AC.pattern(NAME))


def _t(torch, x, tdt, grad=True):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(tdt).cuda().requires_grad_(grad)


def _same_bits(a, b):
    a, b = a.float().cpu().numpy(), b.float().cpu().numpy()
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _inputs(seed, Dv=DV):
    pat = AC.pattern(NAME)
    M, N = pat[0], pat[1]
    return (signed_data(M * D, seed).reshape(M, D), signed_data(N * D, seed + 1).reshape(N, D),
            signed_data(N * Dv, seed + 2).reshape(N, Dv), signed_data(M * Dv, seed + 3).reshape(M, Dv))


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_gradients_equal_the_composed_attention_bitwise(dtype):
    torch = torch_cuda()
    from bsmr import autograd
    pat, plan = AC.pattern(NAME), _plan()
    tdt = torch.float32 if dtype == F32 else torch.float16
    Q, K, V, dO = _inputs(91)
    scale = D ** -0.5
    tdO = _t(torch, dO, torch.float32, grad=False)
    a = [_t(torch, X, tdt) for X in (Q, K, V)]
    b = [_t(torch, X, tdt) for X in (Q, K, V)]
    Oc = autograd.attention(plan, *a)
    Oc.backward(tdO)
    O, LSE = autograd.attention_fused(plan, *b, return_lse=True)
    assert O.dtype == torch.float32 and tuple(O.shape) == (pat[0], DV)
    assert LSE.dtype == torch.float32 and tuple(LSE.shape) == (pat[0],) and not LSE.requires_grad
    assert O.requires_grad
    saved = O.grad_fn.saved_tensors
    assert len(saved) == 3 and not any(t.numel() == plan.nnz or plan.nnz in t.shape for t in saved)
    assert [t.data_ptr() for t in saved] == [t.data_ptr() for t in b]
    O.backward(tdO, retain_graph=True)
    torch.cuda.synchronize()
    for name, x, y in zip(("dQ", "dK", "dV"), a, b):
        assert y.grad.dtype == tdt and _same_bits(x.grad, y.grad), f"{name} differs from attention's"
    once = [y.grad.clone() for y in b]
    O.backward(tdO)
    torch.cuda.synchronize()
    for name, g1, y in zip(("dQ", "dK", "dV"), once, b):
        assert _same_bits(y.grad, g1 * 2), f"{name}: two backward passes do not accumulate"
    # forward: inside the bound of the float64 reference (on the operands as the kernel sees them)
    ref = AC.attention_ref(pat, Q, K, V, scale, dtype)
    AC.check_bound(O.detach().cpu().numpy(), LSE.cpu().numpy(), ref, f"attention_fused {AC.DTYPE_NAME[dtype]}")
    # without LSE: the same O, one output
    O2 = autograd.attention_fused(plan, *(t.detach() for t in b), scale=scale)
    assert isinstance(O2, torch.Tensor) and _same_bits(O2, O.detach())
    # only some inputs need a gradient
    q = _t(torch, Q, tdt, grad=False)
    v = _t(torch, V, tdt)
    autograd.attention_fused(plan, q, b[1].detach(), v).backward(tdO)
    torch.cuda.synchronize()
    assert q.grad is None and _same_bits(v.grad, once[2])


def _dense_attention(pat, Q, K, V, dO, scale, dt):
    """(O, dQ, dK, dV) of dense masked attention in numpy at precision dt."""
    M, N, rp, ci = pat
    mask = np.zeros((M, N), bool)
    mask[AC.entry_rows(pat), np.asarray(ci, np.int64)] = True
    Q, K, V, dO = (np.asarray(x, dt) for x in (Q, K, V, dO))
    S = np.where(mask, Q @ K.T, dt(-np.inf))
    m = S.max(axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, dt(0))
    T = np.where(mask, np.exp((S - m) * dt(scale)), dt(0))
    den = T.sum(axis=1, keepdims=True)
    W = T / np.where(den == 0, dt(1), den)
    O = W @ V
    dW = dO @ V.T
    r = (W * dW).sum(axis=1, keepdims=True)
    dS = dt(scale) * W * (dW - r)
    return O, dS @ K, dS.T @ Q, W.T @ dO


def test_end_to_end_against_dense_float64_attention():
    torch = torch_cuda()
    from bsmr import autograd
    pat, plan = AC.pattern(NAME), _plan()
    scale = D ** -0.5
    Q, K, V, dO = _inputs(81)
    ref = _dense_attention(pat, Q, K, V, dO, scale, np.float64)
    f32 = _dense_attention(pat, Q, K, V, dO, scale, np.float32)
    tQ, tK, tV = (_t(torch, X, torch.float32) for X in (Q, K, V))
    O = autograd.attention_fused(plan, tQ, tK, tV)
    O.backward(torch.from_numpy(dO).cuda())
    torch.cuda.synchronize()
    failures = []
    for name, g, r, c in zip(("O", "dQ", "dK", "dV"), (O.detach(), tQ.grad, tK.grad, tV.grad), ref, f32):
        top = np.abs(r).max()
        cpu_err = np.abs(c.astype(np.float64) - r).max() / top
        gpu_err = np.abs(g.cpu().numpy().astype(np.float64) - r).max() / top
        print(f"ATTENTION_FUSED {name}: float32 CPU error {cpu_err:.3e}, GPU error {gpu_err:.3e}, "
              f"tolerance {8 * cpu_err:.3e}")
        assert cpu_err > 0
        if not gpu_err <= 8 * cpu_err:
            failures.append((name, gpu_err, 8 * cpu_err))
    assert not failures, failures


def test_validation_raises_before_any_launch():
    torch = torch_cuda()
    from bsmr import autograd
    pat = AC.pattern("empty")
    plan = AC.make_plan(pat)
    M, N = pat[0], pat[1]
    z = functools.partial(torch.zeros, dtype=torch.float32, device="cuda")
    h = functools.partial(torch.zeros, dtype=torch.float16, device="cuda")
    for scale in (0.0, -0.5, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="scale"):
            autograd.attention_fused(plan, z((M, 32)), z((N, 32)), z((N, 32)), scale=scale)
    with pytest.raises(ValueError, match="sddmm"):
        autograd.attention_fused(plan, z((M, 32)), z((N, 16)), z((N, 32)))
    with pytest.raises(ValueError, match="sddmm"):
        autograd.attention_fused(plan, z((M, 32)).cpu(), z((N, 32)), z((N, 32)))
    with pytest.raises(ValueError, match="sddmm"):
        autograd.attention_fused(plan, h((M, 48)), h((N, 48)), h((N, 32)))
    with pytest.raises(ValueError, match="spmm"):
        autograd.attention_fused(plan, z((M, 32)), z((N, 32)), z((N + 1, 32)))
    with pytest.raises(ValueError, match="spmm"):
        autograd.attention_fused(plan, z((M, 32)), z((N, 32)), z((N, 64))[:, ::2])
    with pytest.raises(ValueError, match="attention_fused"):
        autograd.attention_fused(plan, z(M), z((N, 32)), z((N, 32)))
    with pytest.raises(ValueError, match="attention_fused.*dtype"):
        autograd.attention_fused(plan, z((M, 32)), z((N, 32)), h((N, 32)))
    with pytest.raises(ValueError, match="spmm"):
        autograd.attention_fused(plan, h((M, 32)), h((N, 32)), h((N, 40)))
    cap = AC.limits()["max_row_bytes"]
    with pytest.raises(ValueError, match="attention_fused.*bytes"):
        autograd.attention_fused(plan, z((M, cap // 4 + 16)), z((N, cap // 4 + 16)), z((N, 32)))
    with pytest.raises(ValueError, match="attention_fused.*bytes"):
        autograd.attention_fused(plan, h((M, 32)), h((N, 32)), h((N, cap // 2 + 32)))
    # nothing was launched or built
    assert not plan.attention_prepared(32, 32) and not plan.softmax_prepared() and not plan.spmm_prepared(32, 3)
