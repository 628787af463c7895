"""GPU: bsmr.autograd.sddmm, the torch.autograd binding of the plan-based SDDMM.

loss = (sddmm(plan, A, B) * W).sum() with W standard normal; A.grad and B.grad against a float64
CPU torch autograd of ((A @ B.T)[rows, cols] * W).sum() on the same (fp16 / bf16 rounded)
operands. Bound per element: 2 n 2^-24 sum|w x| + 1e-6 (n the destination's list length: an
n-term fp32 sum of once-rounded products, as tests/test_gpu_spmm.py), plus eps |ref| for the
final cast of half gradients (eps = 2^-11 fp16, 2^-8 bf16: half an ulp of the result format).
"""
import numpy as np
import pytest

from bsmr import BF16, F16, F32, Plan, make_data
from gpu_util import half_values, torch_cuda
from spmm_cases import entry_rows, pattern, signed_bound, spmm_ref

pytestmark = pytest.mark.gpu

FREE = 288 * 1024 ** 3
EPS = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}


def _tdt(torch, dtype):
    return {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}[dtype]


def _operands(name, K, dtype):
    M, N, _, ci = pattern(name)
    A = (make_data(M * K) - np.float32(1.0)).reshape(M, K)
    B = (make_data(N * K)[::-1].copy() - np.float32(1.0)).reshape(N, K)
    if dtype != F32:
        A, B = half_values(A, dtype), half_values(B, dtype)
    W = np.random.default_rng(23).standard_normal(len(ci)).astype(np.float32)
    return A, B, W


def _plan(name):
    M, N, rp, ci = pattern(name)
    return Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE)


@pytest.mark.parametrize("K,dtype", [(64, F32), (128, F16), (128, BF16)])
@pytest.mark.parametrize("name", ["zipf", "empty"])
def test_gradients_match_float64_autograd(name, K, dtype):
    torch = torch_cuda()
    import bsmr.autograd as BA

    pat = pattern(name)
    M, N, rp, ci = pat
    A, B, W = _operands(name, K, dtype)
    plan = _plan(name)
    dA = torch.from_numpy(A).cuda().to(_tdt(torch, dtype)).requires_grad_()
    dB = torch.from_numpy(B).cuda().to(_tdt(torch, dtype)).requires_grad_()
    dW = torch.from_numpy(W).cuda()
    P = BA.sddmm(plan, dA, dB)
    assert P.shape == (len(ci),) and P.dtype == torch.float32
    (P * dW).sum().backward()
    torch.cuda.synchronize()
    assert dA.grad.dtype == dA.dtype and dB.grad.dtype == dB.dtype
    assert dA.grad.shape == (M, K) and dB.grad.shape == (N, K)

    # float64 CPU autograd of the dense formulation
    cA = torch.from_numpy(A).double().requires_grad_()
    cB = torch.from_numpy(B).double().requires_grad_()
    rows = torch.from_numpy(entry_rows(M, rp))
    cols = torch.from_numpy(ci.astype(np.int64))
    ((cA @ cB.T)[rows, cols] * torch.from_numpy(W).double()).sum().backward()
    for what, got, ref, side, X in (("dA", dA.grad, cA.grad, 1, B), ("dB", dB.grad, cB.grad, 2, A)):
        ref = ref.numpy()
        _, S, n = spmm_ref(pat, side, W, X)
        bound = signed_bound(S, n) + EPS[dtype] * np.abs(ref)
        err = np.abs(got.float().cpu().numpy().astype(np.float64) - ref)
        print(f"{name} K={K} dtype={dtype} {what}: max err / bound = {float((err / bound).max()):.3f}")
        assert np.isfinite(err).all()
        assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements over the bound"


def test_only_the_needed_side_runs():
    torch = torch_cuda()
    import bsmr.autograd as BA

    name, K = "empty", 64
    A, B, W = _operands(name, K, F32)
    dW = torch.from_numpy(W).cuda()
    for needs_a in (True, False):
        plan = _plan(name)
        dA = torch.from_numpy(A).cuda().requires_grad_(needs_a)
        dB = torch.from_numpy(B).cuda().requires_grad_(not needs_a)
        (BA.sddmm(plan, dA, dB) * dW).sum().backward()
        torch.cuda.synchronize()
        assert (dA.grad is not None) == needs_a and (dB.grad is not None) == (not needs_a)
        assert plan.spmm_prepared(K, 1) == needs_a
        assert plan.spmm_prepared(K, 2) == (not needs_a)


def test_bad_operands_raise_before_any_launch():
    torch = torch_cuda()
    import bsmr.autograd as BA

    name, K = "empty", 64
    M, N, _, _ = pattern(name)
    plan = _plan(name)
    A = torch.zeros((M, 2 * K), device="cuda")[:, ::2]  # (M, K), not contiguous
    B = torch.zeros((N, K), device="cuda")
    assert not A.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        BA.sddmm(plan, A, B)
    with pytest.raises(ValueError):
        BA.sddmm(plan, A.contiguous().half(), B)           # two dtypes
    with pytest.raises(ValueError):
        BA.sddmm(plan, A.contiguous().double(), B.double())  # unsupported dtype
    with pytest.raises(ValueError):
        BA.sddmm(plan, A.contiguous().cpu(), B)             # not on the device
    with pytest.raises(ValueError):
        BA.sddmm(plan, A.contiguous()[:-1], B)              # wrong shape
    with pytest.raises(ValueError):
        BA.sddmm(plan, torch.zeros((M, 24), device="cuda"), torch.zeros((N, 24), device="cuda"))
    assert not plan.spmm_prepared(K, 1) and not plan.spmm_prepared(K, 2)
