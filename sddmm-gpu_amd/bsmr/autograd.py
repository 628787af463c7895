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
    attention_fused_heads(plan, Q, K, V)   attention_fused with backward="fused" over (H, M, D) or
                                     (B, H, M, D) operands with any strides (views of a
                                     (B, M, H D) projection, an expanded K / V) in one
                                     Plan.attention_heads call and one Plan.attention_backward_heads call

Every direction is the library's HIP kernels on torch.cuda.current_stream(); torch only owns the
tensors. Importing this module imports torch (`import bsmr` alone does not).
"""
import torch

from . import BF16, F16, F32, attention_heads_limits, attention_layout_check, attention_limits

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


def _validate_heads(plan, Q, K, V):
    """The checks of attention_fused_heads, before any launch or build. Returns (lead, D, Dv, dtype):
    lead = (H,) or (B, H)."""
    who = "attention_fused_heads"
    for name, X in (("Q", Q), ("K", K), ("V", V)):
        if not isinstance(X, torch.Tensor):
            raise ValueError(f"{who}: {name} must be a torch tensor")
        if not X.is_cuda:
            raise ValueError(f"{who}: {name} must be a device tensor, got {X.device}")
        if X.dtype not in _DTYPES:
            raise ValueError(f"{who}: {name} must be float32, float16 or bfloat16, got {X.dtype}")
        if X.dim() not in (3, 4):
            raise ValueError(f"{who}: {name} must be (H, rows, W) or (B, H, rows, W), got {tuple(X.shape)}")
    if not (Q.dtype == K.dtype == V.dtype):
        raise ValueError(f"{who}: Q ({Q.dtype}), K ({K.dtype}) and V ({V.dtype}) must share one dtype")
    if not (Q.device == K.device == V.device):
        raise ValueError(f"{who}: Q ({Q.device}), K ({K.device}) and V ({V.device}) must share one device")
    lead, D, Dv = tuple(Q.shape[:-2]), Q.shape[-1], V.shape[-1]
    for name, X, rows, W in (("Q", Q, plan.M, D), ("K", K, plan.N, D), ("V", V, plan.N, Dv)):
        if tuple(X.shape) != lead + (rows, W):
            raise ValueError(f"{who}: {name} must be {lead + (rows, W)}, got {tuple(X.shape)}")
    lim = attention_heads_limits()
    B, H = (1,) * (2 - len(lead)) + lead
    if not (1 <= B <= lim["max_batches"] and 1 <= H <= lim["max_heads"]):
        raise ValueError(f"{who}: batch = {B} and heads = {H} must be 1 .. {lim['max_batches']} and 1 .. {lim['max_heads']}")
    mult = 16 if Q.dtype == torch.float32 else 32
    if D == 0 or D % mult or Dv == 0 or Dv % 16:
        raise ValueError(f"{who}: D = {D} must be a positive multiple of {mult} for {Q.dtype} and Dv = {Dv} of 16")
    cap = attention_limits()["max_row_bytes"]
    if max(D, Dv) * Q.element_size() > cap:
        raise ValueError(f"{who}: rows of D = {D} / Dv = {Dv} {Q.dtype} exceed {cap} bytes")
    for name, X, rows, W in (("Q", Q, plan.M, D), ("K", K, plan.N, D), ("V", V, plan.N, Dv)):
        if X.stride(-1) != 1 or min(X.stride()) < 0:
            raise ValueError(f"{who}: {name} must have a contiguous last dimension, got strides {tuple(X.stride())}")
        bad = attention_layout_check(X, B, H, rows, W, X.element_size(), False)
        if bad is not None:
            raise ValueError(f"{who}: {name}: {bad}")
    return lead, D, Dv, _DTYPES[Q.dtype]


def _dense_like(X, shape, dtype=torch.float32):
    """An uninitialised dense tensor of `shape` whose dimensions are laid out in X's dimension order
    (by stride, descending; an expanded or size-1 dimension keeps its standard place)."""
    nd = len(shape)
    if any(st == 0 and n > 1 for st, n in zip(X.stride(), X.shape)):
        return torch.empty(shape, dtype=dtype, device=X.device)
    order = sorted(range(nd - 1), key=lambda i: (-X.stride(i), i)) + [nd - 1]
    inv = [order.index(i) for i in range(nd)]
    return torch.empty([shape[i] for i in order], dtype=dtype, device=X.device).permute(inv)


class _AttentionFusedHeads(torch.autograd.Function):
    """attention_fused_heads: the forward always takes LSE and saves Q, K, V, O and LSE; the backward
    is one Plan.attention_backward_heads call."""

    @staticmethod
    def forward(ctx, Q, K, V, plan, scale, want_lse, checked):
        lead, D, Dv, dtype = checked  # (_validate_heads, run once by attention_fused_heads)
        B, H = (1,) * (2 - len(lead)) + lead
        O = _dense_like(Q, lead + (plan.M, Dv))
        lse = torch.empty(lead + (plan.M,), dtype=torch.float32, device=Q.device)
        plan.attention_heads(B, H, Q, K, V, D, Dv, O, lse.data_ptr(), scale, stream=_stream(), dtype=dtype)
        ctx.plan, ctx.scale, ctx.dims = plan, scale, (B, H, D, Dv, dtype)
        ctx.save_for_backward(Q, K, V, O, lse)
        if not want_lse:
            return O
        ctx.mark_non_differentiable(lse)
        return O, lse

    @staticmethod
    def backward(ctx, grad, *_):
        Q, K, V, O, lse = ctx.saved_tensors
        plan = ctx.plan
        B, H, D, Dv, dtype = ctx.dims
        if not any(ctx.needs_input_grad[:3]):
            return None, None, None, None, None, None, None
        dO = grad if grad.dtype == torch.float32 else grad.float()
        if dO.stride(-1) != 1 or attention_layout_check(dO, B, H, plan.M, Dv, 4, False) is not None:
            dO = dO.contiguous()
        out = [_dense_like(X, X.shape) if need else None for need, X in zip(ctx.needs_input_grad[:3], (Q, K, V))]
        plan.attention_backward_heads(B, H, Q, K, V, O, dO, lse.data_ptr(), D, Dv, out[0], out[1], out[2], ctx.scale,
                                      stream=_stream(), dtype=dtype)
        gQ, gK, gV = (None if t is None else t.to(X.dtype) for t, X in zip(out, (Q, K, V)))
        return gQ, gK, gV, None, None, None, None


def attention_fused_heads(plan, Q, K, V, scale=None, return_lse=False):
    """attention_fused(..., backward="fused") over heads and an optional batch of one sparsity
    pattern: Q (H, M, D) or (B, H, M, D), K and V the same with N rows (V of width Dv). Returns O
    (..., M, Dv) float32 and, with return_lse=True, LSE (..., M) float32, non-differentiable.

    Any strides with a contiguous last dimension are taken as they are, without a copy:
    x.view(B, M, H, D).transpose(1, 2) of a (B, M, H D) projection, K.expand(B, H, N, D) of one K
    shared by all heads. The layout rules are the library's (bsmr.attention_layout_check: 16-byte
    aligned pointers and strides, row stride >= the row width); a violation, like a wrong shape,
    dtype or dimension, raises ValueError before any launch or build.

    O is allocated dense in Q's dimension order, so for a Q that came from (B, M, H D),
    O.transpose(1, 2).reshape(B, M, H Dv) is a view. One Plan.attention_heads call (at most two
    launches) forward; the forward always takes LSE and saves Q, K, V, O and LSE, and the backward
    is one Plan.attention_backward_heads call (at most five launches) that passes NULL for the
    outputs no input needs. Gradients are dense, in their input's dimension order, and cast to the
    input's dtype; for an expanded input they are dense in standard order and torch's expand
    backward sums them. Slice (b, h) of every result equals, bit for bit, attention_fused(...,
    backward="fused") on contiguous copies of that slice."""
    if scale is None:
        if not isinstance(Q, torch.Tensor) or Q.dim() not in (3, 4) or Q.shape[-1] == 0:
            raise ValueError("attention_fused_heads: Q must be an (H, M, D) or (B, H, M, D) tensor with D > 0")
        scale = Q.shape[-1] ** -0.5
    scale = _valid_scale("attention_fused_heads", scale)
    checked = _validate_heads(plan, Q, K, V)
    return _AttentionFusedHeads.apply(Q, K, V, plan, scale, bool(return_lse), checked)
