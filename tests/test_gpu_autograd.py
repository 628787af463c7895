"""GPU: bsmr.autograd.sddmm, the torch.autograd binding of the plan-based SDDMM.

loss = (sddmm(plan, A, B) * W).sum() with W standard normal; A.grad and B.grad against a float64
CPU torch autograd of ((A @ B.T)[rows, cols] * W).sum() on the same (fp16 / bf16 rounded)
operands. Bound per element: 2 n 2^-24 sum|w x| + 1e-6 (n the destination's list length: an
n-term fp32 sum of once-rounded products, as tests/test_gpu_spmm.py), plus eps |ref| for the
final cast of half gradients (eps = 2^-11 fp16, 2^-8 bf16: half an ulp of the result format).

On grid data (tests/spmm_cases.py) the gradients are exact: fp32 equals the float64 reference bit
for bit, fp16 / bf16 equal it cast once by torch; also for an expanded and a strided grad_output
and accumulated over two backward passes. fp16 / bf16 at K = 48 (no forward launch) raise
ValueError from sddmm() before any launch or list build.
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


ROW_BLOCK_KD = [(64, F32), (128, F16), (128, BF16)]  # rows of 256 bytes: the row-block forward launch
KD_IDS = ["K64_f32", "K128_f16", "K128_bf16"]


def _grid_leaves(torch, name, K, dtype):
    from sddmm_cases import grid_data
    M, N, _, _ = pattern(name)
    A = grid_data(M * K, 41).reshape(M, K)
    B = grid_data(N * K, 42).reshape(N, K)
    dA = torch.from_numpy(A).cuda().to(_tdt(torch, dtype)).requires_grad_()
    dB = torch.from_numpy(B).cuda().to(_tdt(torch, dtype)).requires_grad_()
    return A, B, dA, dB


def _assert_grad_exact(torch, got, pat, side, G, X, dtype, what, times=1):
    """got == times x the exact S(G) X (side 1) / S(G)^T X (side 2), cast to the operand's type by
    torch: on grid data the fp32 value is exact, so that cast is the only rounding (|value| <=
    16 x 2048 stays inside fp16's range)."""
    Yr, _, _ = spmm_ref(pat, side, G, X)
    exact = (times * Yr).astype(np.float32)
    assert np.array_equal(exact.astype(np.float64), times * Yr)
    want = torch.from_numpy(exact).to(_tdt(torch, dtype))
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = int((got.cpu() != want).sum())
    assert bad == 0, f"{what}: {bad} elements differ from the exact gradient"


@pytest.mark.parametrize("K,dtype", ROW_BLOCK_KD, ids=KD_IDS)
@pytest.mark.parametrize("name", ["zipf", "hub"])
def test_grid_gradients_are_exact(name, K, dtype):
    torch = torch_cuda()
    import bsmr.autograd as BA
    from spmm_cases import grid_values

    pat = pattern(name)
    A, B, dA, dB = _grid_leaves(torch, name, K, dtype)
    W = grid_values(len(pat[3]), 43)
    plan = _plan(name)
    (BA.sddmm(plan, dA, dB) * torch.from_numpy(W).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert any(plan.stats()["rb_items"])
    _assert_grad_exact(torch, dA.grad, pat, 1, W, B, dtype, f"{name} K={K} dtype={dtype} dA")
    _assert_grad_exact(torch, dB.grad, pat, 2, W, A, dtype, f"{name} K={K} dtype={dtype} dB")


@pytest.mark.parametrize("K,dtype", ROW_BLOCK_KD, ids=KD_IDS)
def test_backward_takes_any_grad_output_layout(K, dtype):
    torch = torch_cuda()
    import bsmr.autograd as BA
    from spmm_cases import grid_values

    name = "zipf"
    pat = pattern(name)
    nnz = len(pat[3])
    A, B, dA, dB = _grid_leaves(torch, name, K, dtype)
    plan = _plan(name)
    # an expanded grad_output (every stride 0)
    BA.sddmm(plan, dA, dB).sum().backward()
    ones = np.ones(nnz, np.float32)
    _assert_grad_exact(torch, dA.grad, pat, 1, ones, B, dtype, "expanded dA")
    _assert_grad_exact(torch, dB.grad, pat, 2, ones, A, dtype, "expanded dB")
    # a non-contiguous one
    G2 = grid_values(2 * nnz, 44)
    dG2 = torch.from_numpy(G2).cuda()
    assert not dG2[::2].is_contiguous()
    gA, gB = torch.autograd.grad(BA.sddmm(plan, dA, dB), (dA, dB), dG2[::2])
    _assert_grad_exact(torch, gA, pat, 1, G2[::2], B, dtype, "strided dA")
    _assert_grad_exact(torch, gB, pat, 2, G2[::2], A, dtype, "strided dB")
    # two backward passes over one graph accumulate exactly twice the gradient
    dA.grad = dB.grad = None
    W = G2[1::2].copy()
    loss = (BA.sddmm(plan, dA, dB) * torch.from_numpy(W).cuda()).sum()
    loss.backward(retain_graph=True)
    loss.backward()
    torch.cuda.synchronize()
    _assert_grad_exact(torch, dA.grad, pat, 1, W, B, dtype, "accumulated dA", times=2)
    _assert_grad_exact(torch, dB.grad, pat, 2, W, A, dtype, "accumulated dB", times=2)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_half_k48_is_refused_before_any_launch(dtype):
    """fp16 / bf16 at K = 48 pass the K % 16 rule of the gradients, but no forward launch takes
    them (launch_select.cpp validate_launch_k: a multiple of 32): sddmm() raises ValueError itself,
    no P is returned, neither side's lists are built and no forward layout exists."""
    torch = torch_cuda()
    import bsmr.autograd as BA

    name, K = "empty", 48
    M, N, _, _ = pattern(name)
    plan = _plan(name)
    A = torch.zeros((M, K), dtype=_tdt(torch, dtype), device="cuda", requires_grad=True)
    B = torch.zeros((N, K), dtype=_tdt(torch, dtype), device="cuda", requires_grad=True)
    P = None
    with pytest.raises(ValueError, match="multiple of 32"):
        P = BA.sddmm(plan, A, B)
    assert P is None
    empty = dict(segments=0, split_dsts=0, partials=0, max_list=0, chunk=0)
    assert plan.spmm_stats(1) == empty and plan.spmm_stats(2) == empty
    assert not plan.spmm_prepared(K, 1) and not plan.spmm_prepared(K, 2) and not plan.prepared(K, dtype)
    # the same K in fp32 is a column-major launch and differentiates
    A32 = torch.zeros((M, K), device="cuda", requires_grad=True)
    BA.sddmm(plan, A32, torch.zeros((N, K), device="cuda")).sum().backward()
    assert A32.grad.shape == (M, K) and plan.spmm_prepared(K, 1)


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
