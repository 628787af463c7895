"""torch.autograd binding of the plan-based SDDMM: P = sddmm(plan, A, B) with gradients.

    forward   P[idx(i,j)] = dot(A[i,:], B[j,:])                 Plan.sddmm
    backward  dA = S(G) B (Plan.spmm), dB = S(G)^T A (Plan.spmm_t), G = dL/dP

and, over the same plan, the row softmax, the SpMM and their composition into sparse attention:

    softmax(plan, P, scale)      W = per-row softmax(scale P)     Plan.softmax / softmax_backward
    spmm(plan, V, X)             Y = S(V) X                        Plan.spmm; dV = Plan.sddmm(dY, X),
                                                                   dX = Plan.spmm_t(V, dY)
    attention(plan, Q, K, V)     spmm(softmax(sddmm(Q, K), scale), V)
    attention_fused(plan, Q, K, V)   the same O from one fused forward launch (Plan.attention) that
                                     keeps no nnz-sized tensor; the backward recomputes P and W, or
                                     (backward="fused") is one Plan.attention_backward call that
                                     holds no nnz-sized tensor either

Every direction is the library's HIP kernels on torch.cuda.current_stream(); torch only owns the
tensors. Importing this module imports torch (`import bsmr` alone does not).
"""
import torch

from . import BF16, F16, F32, attention_limits

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


def _valid_scale(who, scale):
    try:
        s = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: scale must be a number, got {scale!r}") from None
    if not (s > 0.0) or s == float("inf"):
        raise ValueError(f"{who}: scale = {scale!r} must be finite and > 0")
    return s


def _validate_values(who, name, plan, P):
    """A vector of one fp32 value per stored entry, in CSR order."""
    if not isinstance(P, torch.Tensor):
        raise ValueError(f"{who}: {name} must be a torch tensor")
    if not P.is_cuda:
        raise ValueError(f"{who}: {name} must be a device tensor, got {P.device}")
    if P.dtype != torch.float32:
        raise ValueError(f"{who}: {name} must be float32, got {P.dtype}")
    if P.dim() != 1 or P.shape[0] != plan.nnz:
        raise ValueError(f"{who}: {name} must be ({plan.nnz},), got {tuple(P.shape)}")
    if not P.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")


def _launchable(t):
    """The launch wants a valid pointer even for a plan without entries."""
    return t if t.shape[0] else torch.zeros(1, dtype=torch.float32, device=t.device)


class _Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, plan, scale):
        W = torch.empty(max(plan.nnz, 1), dtype=torch.float32, device=P.device)
        plan.softmax(_launchable(P).data_ptr(), W.data_ptr(), scale, stream=_stream())
        W = W[:plan.nnz]
        ctx.plan, ctx.scale = plan, scale
        ctx.save_for_backward(W)
        return W

    @staticmethod
    def backward(ctx, grad):
        (W,) = ctx.saved_tensors
        plan = ctx.plan
        G = grad.contiguous().float()
        gP = torch.empty(max(plan.nnz, 1), dtype=torch.float32, device=W.device)
        plan.softmax_backward(_launchable(W).data_ptr(), _launchable(G).data_ptr(), gP.data_ptr(), ctx.scale,
                              stream=_stream())
        return gP[:plan.nnz], None, None


def softmax(plan, P, scale=1.0):
    """W (nnz,) float32 = per row of the plan's pattern, softmax(scale * P) over the row's stored
    entries (Plan.softmax), differentiable in P (Plan.softmax_backward). P: (nnz,) float32
    contiguous device tensor in CSR order; scale finite and > 0. Errors raise ValueError before
    any launch."""
    _validate_values("softmax", "P", plan, P)
    return _Softmax.apply(P, plan, _valid_scale("softmax", scale))


def _validate_dense(plan, X):
    """The dense operand of spmm: (N, K) of a supported dtype; returns (K, dtype)."""
    if not isinstance(X, torch.Tensor):
        raise ValueError("spmm: X must be a torch tensor")
    if not X.is_cuda:
        raise ValueError(f"spmm: X must be a device tensor, got {X.device}")
    if X.dtype not in _DTYPES:
        raise ValueError(f"spmm: X must be float32, float16 or bfloat16, got {X.dtype}")
    if X.dim() != 2 or X.shape[0] != plan.N:
        raise ValueError(f"spmm: X must be ({plan.N}, K), got {tuple(X.shape)}")
    if not X.is_contiguous():
        raise ValueError("spmm: X must be contiguous")
    K = X.shape[1]
    if K == 0 or K % 16:
        raise ValueError(f"spmm: K = {K} must be a positive multiple of 16")
    return K, _DTYPES[X.dtype]


def _validate_spmm(plan, V, X):
    _validate_values("spmm", "V", plan, V)
    K, dtype = _validate_dense(plan, X)
    if V.device != X.device:
        raise ValueError(f"spmm: V ({V.device}) and X ({X.device}) must share one device")
    return K, dtype


class _Spmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, V, X, plan):
        K, dtype = _validate_spmm(plan, V, X)
        Y = torch.empty((plan.M, K), dtype=torch.float32, device=X.device)
        plan.spmm(_launchable(V).data_ptr(), X.data_ptr(), K, Y.data_ptr(), stream=_stream(), dtype=dtype)
        ctx.plan, ctx.K = plan, K
        ctx.save_for_backward(V, X)
        return Y

    @staticmethod
    def backward(ctx, grad):
        V, X = ctx.saved_tensors
        plan, K = ctx.plan, ctx.K
        dY = grad.contiguous().float()
        gV = gX = None
        if ctx.needs_input_grad[0]:
            # fp32 SDDMM of dY (fp32) with X: a half X is cast up once
            gV = torch.empty(max(plan.nnz, 1), dtype=torch.float32, device=X.device)
            plan.sddmm(dY.data_ptr(), X.float().data_ptr(), K, gV.data_ptr(), stream=_stream())
            gV = gV[:plan.nnz]
        if ctx.needs_input_grad[1]:
            gX = torch.empty((plan.N, K), dtype=torch.float32, device=X.device)
            plan.spmm_t(_launchable(V).data_ptr(), dY.data_ptr(), K, gX.data_ptr(), stream=_stream())
            gX = gX.to(X.dtype)
        return gV, gX, None


def spmm(plan, V, X):
    """Y (M, K) float32 = S(V) X, the plan's pattern with values V times the dense X (Plan.spmm),
    differentiable in both: dV = the plan's sampled dY @ X.T (Plan.sddmm, in fp32: a float16 /
    bfloat16 X is cast up to float32 once for it), dX = S(V)^T dY (Plan.spmm_t, returned in X's
    dtype). V: (nnz,) float32 in CSR order; X: (N, K) float32, float16 or bfloat16, K a positive
    multiple of 16; contiguous tensors of one device. Errors raise ValueError before any launch."""
    _validate_spmm(plan, V, X)
    return _Spmm.apply(V, X, plan)


def attention(plan, Q, K, V, scale=None):
    """O (M, Dv) float32 = softmax(scale * S .* (Q @ K.T)) @ V over the plan's pattern, exactly
    spmm(plan, softmax(plan, sddmm(plan, Q, K), scale), V) and nothing more; scale = 1 / sqrt(D)
    by default (D = Q.shape[1]). Q: (M, D), K: (N, D), V: (N, Dv); each op's own rules apply."""
    if scale is None:
        if not isinstance(Q, torch.Tensor) or Q.dim() != 2 or Q.shape[1] == 0:
            raise ValueError("attention: Q must be an (M, D) tensor with D > 0")
        scale = Q.shape[1] ** -0.5
    scale = _valid_scale("attention", scale)
    # every operand is checked before the first launch (each op checks its own again)
    _validate(plan, Q, K)
    _validate_dense(plan, V)
    if V.device != Q.device:
        raise ValueError(f"spmm: V ({V.device}) and Q ({Q.device}) must share one device")
    return spmm(plan, softmax(plan, sddmm(plan, Q, K), scale), V)


def _validate_fused(plan, Q, K, V):
    """attention's checks, one dtype for all three operands and rows within the fused kernel's byte
    cap. Returns (D, Dv, dtype)."""
    D, dtype = _validate(plan, Q, K)
    Dv, vdtype = _validate_dense(plan, V)
    if V.device != Q.device:
        raise ValueError(f"spmm: V ({V.device}) and Q ({Q.device}) must share one device")
    if vdtype != dtype:
        raise ValueError(f"attention_fused: V ({V.dtype}) must share the dtype of Q and K ({Q.dtype})")
    cap = attention_limits()["max_row_bytes"]
    if max(D, Dv) * Q.element_size() > cap:
        raise ValueError(f"attention_fused: rows of D = {D} / Dv = {Dv} {Q.dtype} exceed {cap} bytes")
    return D, Dv, dtype


class _AttentionFused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Q, K, V, plan, scale, want_lse):
        D, Dv, dtype = _validate_fused(plan, Q, K, V)
        O = torch.empty((plan.M, Dv), dtype=torch.float32, device=Q.device)
        lse = torch.empty(plan.M, dtype=torch.float32, device=Q.device) if want_lse else None
        plan.attention(Q.data_ptr(), K.data_ptr(), V.data_ptr(), D, Dv, O.data_ptr(),
                       lse.data_ptr() if want_lse else 0, scale, stream=_stream(), dtype=dtype)
        ctx.plan, ctx.scale, ctx.dims = plan, scale, (D, Dv, dtype)
        ctx.save_for_backward(Q, K, V)
        if not want_lse:
            return O
        ctx.mark_non_differentiable(lse)
        return O, lse

    @staticmethod
    def backward(ctx, grad, *_):
        Q, K, V = ctx.saved_tensors
        plan, scale = ctx.plan, ctx.scale
        D, Dv, dtype = ctx.dims
        s = _stream()
        vec = lambda: torch.empty(max(plan.nnz, 1), dtype=torch.float32, device=Q.device)  # noqa: E731
        dO = grad.contiguous().float()
        # P and W again, by the launches of the composed forward
        P, W = vec(), vec()
        plan.sddmm(Q.data_ptr(), K.data_ptr(), D, P.data_ptr(), stream=s, dtype=dtype)
        plan.softmax(P.data_ptr(), W.data_ptr(), scale, stream=s)
        # from here on exactly the launches of attention's backward (_Spmm, _Softmax, _Sddmm)
        need_qk = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        gQ = gK = gV = None
        if need_qk:
            gW = vec()
            plan.sddmm(dO.data_ptr(), V.float().data_ptr(), Dv, gW.data_ptr(), stream=s)
        if ctx.needs_input_grad[2]:
            gV = torch.empty((plan.N, Dv), dtype=torch.float32, device=Q.device)
            plan.spmm_t(W.data_ptr(), dO.data_ptr(), Dv, gV.data_ptr(), stream=s)
            gV = gV.to(V.dtype)
        if need_qk:
            gP = vec()
            plan.softmax_backward(W.data_ptr(), gW.data_ptr(), gP.data_ptr(), scale, stream=s)
            if ctx.needs_input_grad[0]:
                gQ = torch.empty((plan.M, D), dtype=torch.float32, device=Q.device)
            if ctx.needs_input_grad[1]:
                gK = torch.empty((plan.N, D), dtype=torch.float32, device=Q.device)
            plan.sddmm_backward(gP.data_ptr(), Q.data_ptr(), K.data_ptr(), D,
                                gQ.data_ptr() if gQ is not None else 0,
                                gK.data_ptr() if gK is not None else 0, stream=s, dtype=dtype)
            gQ = None if gQ is None else gQ.to(Q.dtype)
            gK = None if gK is None else gK.to(K.dtype)
        return gQ, gK, gV, None, None, None


class _AttentionFusedBwd(torch.autograd.Function):
    """attention_fused with backward="fused": the forward always takes LSE and saves Q, K, V, O and
    LSE; the backward is one Plan.attention_backward call."""

    @staticmethod
    def forward(ctx, Q, K, V, plan, scale, want_lse):
        D, Dv, dtype = _validate_fused(plan, Q, K, V)
        O = torch.empty((plan.M, Dv), dtype=torch.float32, device=Q.device)
        lse = torch.empty(max(plan.M, 1), dtype=torch.float32, device=Q.device)
        plan.attention(Q.data_ptr(), K.data_ptr(), V.data_ptr(), D, Dv, O.data_ptr(), lse.data_ptr(), scale,
                       stream=_stream(), dtype=dtype)
        lse = lse[:plan.M]
        ctx.plan, ctx.scale, ctx.dims = plan, scale, (D, Dv, dtype)
        ctx.save_for_backward(Q, K, V, O, lse)
        if not want_lse:
            return O
        ctx.mark_non_differentiable(lse)
        return O, lse

    @staticmethod
    def backward(ctx, grad, *_):
        Q, K, V, O, lse = ctx.saved_tensors
        plan = ctx.plan
        D, Dv, dtype = ctx.dims
        if not any(ctx.needs_input_grad[:3]):
            return None, None, None, None, None, None
        dO = grad.contiguous().float()
        out = [torch.empty(shape, dtype=torch.float32, device=Q.device) if need else None
               for need, shape in zip(ctx.needs_input_grad[:3], ((plan.M, D), (plan.N, D), (plan.N, Dv)))]
        ptr = [0 if t is None else t.data_ptr() for t in out]
        plan.attention_backward(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(),
                                _launchable(lse).data_ptr(), D, Dv, ptr[0], ptr[1], ptr[2], ctx.scale,
                                stream=_stream(), dtype=dtype)
        gQ, gK, gV = (None if t is None else t.to(X.dtype) for t, X in zip(out, (Q, K, V)))
        return gQ, gK, gV, None, None, None


def attention_fused(plan, Q, K, V, scale=None, return_lse=False, backward="recompute"):
    """O (M, Dv) float32 of attention(plan, Q, K, V, scale) from one fused forward launch
    (Plan.attention: no nnz-sized scores or weights are written), and with return_lse=True also
    LSE (M,) float32 = max * scale + ln(sum) per row (-inf for an empty row), returned
    non-differentiable. Q, K and V share one dtype and their rows hold at most
    attention_limits()["max_row_bytes"] bytes; otherwise attention's checks (D a positive multiple
    of 16, of 32 for float16 / bfloat16; Dv of 16), with its ValueErrors, before any launch.

    The forward saves Q, K and V only. The backward recomputes P = Plan.sddmm(Q, K) and W =
    Plan.softmax(P, scale) and then runs exactly the launches of attention's backward; it does not
    read O, so dQ, dK and dV are bitwise equal to those of attention. The price is one more SDDMM
    and softmax in the backward; the gain is that no W (nnz values) is held between forward and
    backward. O itself is summed in another order than attention's and agrees with it within the
    two paths' error bounds, not bit for bit.

    backward="fused": the forward always asks for LSE and saves Q, K, V, O and LSE; the backward is
    one Plan.attention_backward call (at most five launches) that computes dQ, dK and dV per entry
    in registers and allocates no nnz-sized tensor, skipping the side no input needs. Its gradients
    agree with the default path's within the two paths' error bounds, not bit for bit. Any other
    value of `backward` raises ValueError before any launch."""
    if backward not in ("recompute", "fused"):
        raise ValueError(f"attention_fused: backward = {backward!r} must be \"recompute\" or \"fused\"")
    if scale is None:
        if not isinstance(Q, torch.Tensor) or Q.dim() != 2 or Q.shape[1] == 0:
            raise ValueError("attention_fused: Q must be an (M, D) tensor with D > 0")
        scale = Q.shape[1] ** -0.5
    scale = _valid_scale("attention_fused", scale)
    _validate_fused(plan, Q, K, V)
    fn = _AttentionFusedBwd if backward == "fused" else _AttentionFused
    return fn.apply(Q, K, V, plan, scale, bool(return_lse))
