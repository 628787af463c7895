"""GPU: bsmr.autograd.spmm, softmax and attention (the differentiable chain
softmax(scale * S .* (Q K^T)) V on the library's kernels).

* autograd.spmm on grid data (exact in fp32 in any order, tests/spmm_cases.py): Y, dV and dX equal
  the float64 values bit for bit for fp32 X; a half X gives dX equal to the exact value cast once;
* autograd.softmax: forward and backward equal Plan.softmax / Plan.softmax_backward bitwise, and two
  backward passes accumulate;
* attention: the forward and all three gradients are bitwise equal to the hand composition of the
  public ops (Plan.sddmm, Plan.softmax, Plan.spmm and their backward launches), each of which is
  held to its own bounds in its own tests;
* end to end on zipf_shuffled at D = Dv = 32, fp32: O, dQ, dK and dV against a float64 dense masked
  attention on the CPU. Tolerance per tensor, relative to max |ref|: 8 x the error that the same
  dense computation in float32 on the CPU shows against float64 on these inputs (the factor 8 for
  the different summation orders); never taken from the GPU result. Both errors are printed;
* ValueError before any launch for a wrong shape, dtype, device, contiguity, K or scale.
"""
import functools

import numpy as np
import pytest

from bsmr import BF16, F16, F32
from gpu_util import torch_cuda
from sddmm_cases import grid_data, sddmm_ref, signed_data
from softmax_cases import entry_rows, make_plan, pattern, signed_scores
from spmm_cases import grid_values, spmm_ref

pytestmark = pytest.mark.gpu
NAME = "zipf_shuffled"


@functools.lru_cache(maxsize=None)
def _plan():
    return make_plan(pattern(NAME))


def _t(torch, x, dtype=None, grad=True):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().requires_grad_(grad)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint32) == b.view(np.uint32)).all())


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_spmm_on_grid_data_is_exact(dtype):
    torch = torch_cuda()
    from bsmr import autograd
    pat, plan = pattern(NAME), _plan()
    M, N, _, ci = pat
    K = 64
    tdt = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}[dtype]
    V, X, dY = grid_values(len(ci), 3), grid_data(N * K, 4).reshape(N, K), grid_data(M * K, 5).reshape(M, K)
    tV, tX = _t(torch, V), _t(torch, X, tdt)
    Y = autograd.spmm(plan, tV, tX)
    assert Y.dtype == torch.float32 and tuple(Y.shape) == (M, K)
    Y.backward(torch.from_numpy(dY).cuda())
    torch.cuda.synchronize()
    assert (Y.detach().cpu().numpy().astype(np.float64) == spmm_ref(pat, 1, V, X)[0]).all(), "Y"
    want_dV = sddmm_ref(pat, dY, X)[0]
    assert tV.grad.dtype == torch.float32
    assert (tV.grad.cpu().numpy().astype(np.float64) == want_dV).all(), "dV"
    want_dX = spmm_ref(pat, 2, V, dY)[0]
    exact32 = want_dX.astype(np.float32)
    assert (exact32.astype(np.float64) == want_dX).all()
    assert tX.grad.dtype == tdt and tuple(tX.grad.shape) == (N, K)
    cast_once = torch.from_numpy(exact32).to(tdt)
    assert torch.equal(tX.grad.cpu(), cast_once), "dX is not the exact value cast once"


def test_softmax_equals_the_plan_calls_and_accumulates():
    torch = torch_cuda()
    from bsmr import autograd
    pat, plan = pattern(NAME), _plan()
    nnz = len(pat[3])
    s = torch.cuda.current_stream().cuda_stream
    P, G = signed_scores(pat, "wide", 61), signed_data(nnz, 62)
    tP, tG = _t(torch, P), _t(torch, G, grad=False)
    W = autograd.softmax(plan, tP, 0.125)
    W.backward(tG, retain_graph=True)
    torch.cuda.synchronize()
    once = tP.grad.clone()
    W.backward(tG)
    torch.cuda.synchronize()
    dW = torch.empty(nnz, dtype=torch.float32, device="cuda")
    dGP = torch.empty(nnz, dtype=torch.float32, device="cuda")
    plan.softmax(tP.data_ptr(), dW.data_ptr(), 0.125, stream=s)
    plan.softmax_backward(dW.data_ptr(), tG.data_ptr(), dGP.data_ptr(), 0.125, stream=s)
    torch.cuda.synchronize()
    assert _same_bits(W.detach().cpu().numpy(), dW.cpu().numpy())
    assert _same_bits(once.cpu().numpy(), dGP.cpu().numpy())
    assert _same_bits(tP.grad.cpu().numpy(), (dGP * 2).cpu().numpy()), "two backward passes do not accumulate"


def _inputs(torch, pat, D, Dv, seed):
    M, N = pat[0], pat[1]
    Q = signed_data(M * D, seed).reshape(M, D)
    K = signed_data(N * D, seed + 1).reshape(N, D)
    V = signed_data(N * Dv, seed + 2).reshape(N, Dv)
    dO = signed_data(M * Dv, seed + 3).reshape(M, Dv)
    return Q, K, V, dO


def test_attention_is_the_composition_of_the_public_ops():
    torch = torch_cuda()
    from bsmr import autograd
    pat, plan = pattern(NAME), _plan()
    M, N, _, ci = pat
    nnz, D, Dv = len(ci), 32, 48
    Q, K, V, dO = _inputs(torch, pat, D, Dv, 71)
    tQ, tK, tV, tdO = _t(torch, Q), _t(torch, K), _t(torch, V), _t(torch, dO, grad=False)
    O = autograd.attention(plan, tQ, tK, tV)
    O.backward(tdO)
    torch.cuda.synchronize()

    s = torch.cuda.current_stream().cuda_stream
    scale = D ** -0.5
    f = functools.partial(torch.empty, dtype=torch.float32, device="cuda")
    P, W, hO, gW, gV, gP, gQ, gK = f(nnz), f(nnz), f((M, Dv)), f(nnz), f((N, Dv)), f(nnz), f((M, D)), f((N, D))
    p = lambda t: t.data_ptr()  # noqa: E731
    plan.sddmm(p(tQ), p(tK), D, p(P), stream=s)
    plan.softmax(p(P), p(W), scale, stream=s)
    plan.spmm(p(W), p(tV), Dv, p(hO), stream=s)
    plan.sddmm(p(tdO), p(tV), Dv, p(gW), stream=s)       # dW = sampled dO V^T
    plan.spmm_t(p(W), p(tdO), Dv, p(gV), stream=s)       # dV = S(W)^T dO
    plan.softmax_backward(p(W), p(gW), p(gP), scale, stream=s)
    plan.spmm(p(gP), p(tK), D, p(gQ), stream=s)          # dQ = S(dP) K
    plan.spmm_t(p(gP), p(tQ), D, p(gK), stream=s)        # dK = S(dP)^T Q
    torch.cuda.synchronize()
    for name, got, want in (("O", O.detach(), hO), ("dQ", tQ.grad, gQ), ("dK", tK.grad, gK), ("dV", tV.grad, gV)):
        assert _same_bits(got.cpu().numpy(), want.cpu().numpy()), f"{name} differs from the hand composition"
    # scale given explicitly: the same default
    O2 = autograd.attention(plan, tQ.detach(), tK.detach(), tV.detach(), scale=scale)
    assert _same_bits(O2.cpu().numpy(), hO.cpu().numpy())


def _dense_attention(pat, Q, K, V, dO, scale, dt):
    """(O, dQ, dK, dV) of dense masked attention in numpy at precision dt."""
    M, N, rp, ci = pat
    mask = np.zeros((M, N), bool)
    mask[entry_rows(pat), np.asarray(ci, np.int64)] = True
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
    pat, plan = pattern(NAME), _plan()
    D = Dv = 32
    scale = D ** -0.5
    Q, K, V, dO = _inputs(torch, pat, D, Dv, 81)
    ref = _dense_attention(pat, Q, K, V, dO, scale, np.float64)
    f32 = _dense_attention(pat, Q, K, V, dO, scale, np.float32)
    tQ, tK, tV = _t(torch, Q), _t(torch, K), _t(torch, V)
    O = autograd.attention(plan, tQ, tK, tV)
    O.backward(torch.from_numpy(dO).cuda())
    torch.cuda.synchronize()
    got = (O.detach(), tQ.grad, tK.grad, tV.grad)
    failures = []
    for name, g, r, c in zip(("O", "dQ", "dK", "dV"), got, ref, f32):
        top = np.abs(r).max()
        cpu_err = np.abs(c.astype(np.float64) - r).max() / top
        gpu_err = np.abs(g.cpu().numpy().astype(np.float64) - r).max() / top
        print(f"ATTENTION {name}: float32 CPU error {cpu_err:.3e}, GPU error {gpu_err:.3e}, tolerance {8 * cpu_err:.3e}")
        assert cpu_err > 0
        if not gpu_err <= 8 * cpu_err:
            failures.append((name, gpu_err, 8 * cpu_err))
    assert not failures, failures


def test_validation_raises_before_any_launch():
    torch = torch_cuda()
    from bsmr import autograd
    pat = pattern("empty")
    plan = make_plan(pat)
    M, N, _, ci = pat
    nnz = len(ci)
    z = functools.partial(torch.zeros, dtype=torch.float32, device="cuda")
    V, X, P = z(nnz), z((N, 32)), z(nnz)
    bad_spmm = [
        (z(nnz + 1), X), (z((nnz, 1)), X), (V.half(), X), (V.cpu(), X), (z(2 * nnz)[::2], X), (V.cpu().numpy(), X),
        (V, z((N + 1, 32))), (V, z((N, 24))), (V, z((N, 0))), (V, z(N)), (V, X.double()), (V, X.cpu()),
        (V, z((N, 64))[:, ::2]), (V, None),
    ]
    for v, x in bad_spmm:
        with pytest.raises(ValueError, match="spmm"):
            autograd.spmm(plan, v, x)
    for p in (z(nnz + 1), P.half(), P.cpu(), z(2 * nnz)[::2], z((nnz, 1)), None):
        with pytest.raises(ValueError, match="softmax"):
            autograd.softmax(plan, p)
    for scale in (0.0, -0.5, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="scale"):
            autograd.softmax(plan, P, scale)
        with pytest.raises(ValueError, match="scale"):
            autograd.attention(plan, z((M, 32)), z((N, 32)), z((N, 32)), scale=scale)
    with pytest.raises(ValueError, match="sddmm"):
        autograd.attention(plan, z((M, 32)), z((N, 16)), z((N, 32)))
    with pytest.raises(ValueError, match="spmm"):
        autograd.attention(plan, z((M, 32)), z((N, 32)), z((N + 1, 32)))
    with pytest.raises(ValueError, match="attention"):
        autograd.attention(plan, z(M), z((N, 32)), z((N, 32)))
    # nothing was launched or built
    assert not plan.softmax_prepared() and not plan.spmm_prepared(32, 3)
