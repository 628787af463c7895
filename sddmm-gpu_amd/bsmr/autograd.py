"""torch.autograd binding of the plan-based SDDMM: P = sddmm(plan, A, B) with gradients.

    forward   P[idx(i,j)] = dot(A[i,:], B[j,:])                 Plan.sddmm
    backward  dA = S(G) B (Plan.spmm), dB = S(G)^T A (Plan.spmm_t), G = dL/dP

Both directions are the library's HIP kernels on torch.cuda.current_stream(); torch only owns the
tensors. Importing this module imports torch (`import bsmr` alone does not).
"""
import torch

from . import BF16, F16, F32

_DTYPES = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _validate(plan, A, B):
    for name, X, rows in (("A", A, plan.M), ("B", B, plan.N)):
        if not isinstance(X, torch.Tensor):
            raise ValueError(f"sddmm: {name} must be a torch tensor")
        if not X.is_cuda:
            raise ValueError(f"sddmm: {name} must be a device tensor, got {X.device}")
        if X.dtype not in _DTYPES:
            raise ValueError(f"sddmm: {name} must be float32, float16 or bfloat16, got {X.dtype}")
        if X.dim() != 2 or X.shape[0] != rows:
            raise ValueError(f"sddmm: {name} must be ({rows}, K), got {tuple(X.shape)}")
        if not X.is_contiguous():
            raise ValueError(f"sddmm: {name} must be contiguous")
    if A.dtype != B.dtype:
        raise ValueError(f"sddmm: A ({A.dtype}) and B ({B.dtype}) must share one dtype")
    if A.device != B.device:
        raise ValueError(f"sddmm: A ({A.device}) and B ({B.device}) must share one device")
    K = A.shape[1]
    if B.shape[1] != K:
        raise ValueError(f"sddmm: A has K = {K}, B has K = {B.shape[1]}")
    if K == 0 or K % 16:
        raise ValueError(f"sddmm: K = {K} must be a positive multiple of 16")
    # the forward launch's own rule (csrc/launch_select.cpp validate_launch_k): every fp16 / bf16
    # launch takes a multiple of 32 only (the column-major half launch by that rule; row-block,
    # panel-tile and dense-sampled launches exist at multiples of 64 only)
    if A.dtype != torch.float32 and K % 32:
        raise ValueError(f"sddmm: K = {K}: float16 / bfloat16 inputs need K to be a positive multiple of 32")
    return K, _DTYPES[A.dtype]


class _Sddmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, plan):
        K, dtype = _validate(plan, A, B)
        P = torch.empty(max(plan.nnz, 1), dtype=torch.float32, device=A.device)
        plan.sddmm(A.data_ptr(), B.data_ptr(), K, P.data_ptr(), stream=_stream(), dtype=dtype)
        ctx.plan, ctx.K, ctx.dtype = plan, K, dtype
        ctx.save_for_backward(A, B)
        return P[:plan.nnz]

    @staticmethod
    def backward(ctx, grad):
        A, B = ctx.saved_tensors
        plan, K = ctx.plan, ctx.K
        G = grad.contiguous().float()
        if G.shape[0] < 1:  # the launch wants a valid pointer
            G = torch.zeros(1, dtype=torch.float32, device=A.device)
        gA = gB = None
        if ctx.needs_input_grad[0]:
            gA = torch.empty((plan.M, K), dtype=torch.float32, device=A.device)
        if ctx.needs_input_grad[1]:
            gB = torch.empty((plan.N, K), dtype=torch.float32, device=A.device)
        plan.sddmm_backward(G.data_ptr(), A.data_ptr(), B.data_ptr(), K,
                            gA.data_ptr() if gA is not None else 0,
                            gB.data_ptr() if gB is not None else 0,
                            stream=_stream(), dtype=ctx.dtype)
        return (None if gA is None else gA.to(A.dtype), None if gB is None else gB.to(B.dtype), None)


def sddmm(plan, A, B):
    """P (nnz,) float32 = the plan's sampled A @ B.T, differentiable in A and B. A: (M, K), B:
    (N, K) (the header's column-major K x N), contiguous device tensors of one dtype out of
    float32, float16 and bfloat16; K a positive multiple of 16 (float32) or 32 (float16 /
    bfloat16: what the forward launch takes). Shape, dtype, device, contiguity and K errors raise
    ValueError before any launch and before any gather list is built."""
    _validate(plan, A, B)
    return _Sddmm.apply(A, B, plan)
