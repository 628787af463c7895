"""GPU: bsmr.autograd.attention_fused(..., backward="fused"): the forward is the one fused launch with
LSE, the backward one Plan.attention_backward call that holds no nnz-sized tensor. zipf_shuffled,
D = 32, Dv = 48, fp32 and fp16.

* O, dQ, dK and dV against the float64 dense masked attention on the CPU: per tensor 8 x the error
  of the same dense computation in float32 on the CPU, relative to max |ref|, both errors printed
  (the rule of tests/test_gpu_attention_autograd.py; DESIGN.md section 14 records the values). At fp16
  the reference is taken on the operands rounded to fp16, and a gradient, which autograd returns in
  fp16, is held to 8 x the error of the float32 CPU gradient cast to fp16 the same single time: no
  fp16 value can be closer to the reference than that format allows;
* the forward saves Q, K, V, O and LSE and nothing of nnz elements; LSE is returned on request,
  non-differentiable; two backward passes accumulate;
* needs_input_grad subsets (Q only, V only, K and V) give the full call's gradients bit for bit;
* memory, on a dense 512 x 512 pattern at D = Dv = 16 (nnz 4 bytes = 1 MiB, a dense operand 32 KiB):
  torch's peak grows during .backward() by less than nnz 4 bytes with "fused" and by more than
  3 nnz 4 bytes with "recompute" (today's path: the test can tell the two apart);
* an unknown backward= raises ValueError before any launch.
"""
import functools

import numpy as np
import pytest

import attention_cases as AC
from bsmr import F16, F32
from gpu_util import half_values, torch_cuda
from sddmm_cases import signed_data
from test_gpu_attention_fused_autograd import _dense_attention, _inputs, _same_bits, _t

pytestmark = pytest.mark.gpu
NAME = "zipf_shuffled"
D, DV = 32, 48


@functools.lru_cache(maxsize=None)
def _plan():
    return AC.make_plan(AC.pattern(NAME))


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_end_to_end_against_dense_float64_attention(dtype):
    torch = torch_cuda()
    from bsmr import autograd
    pat, plan = AC.pattern(NAME), _plan()
    tdt = torch.float32 if dtype == F32 else torch.float16
    scale = D ** -0.5
    Q, K, V, dO = _inputs(81)
    if dtype != F32:  # the operands as every path sees them
        Q, K, V = (half_values(X, dtype) for X in (Q, K, V))
    ref = _dense_attention(pat, Q, K, V, dO, scale, np.float64)
    f32 = _dense_attention(pat, Q, K, V, dO, scale, np.float32)
    tQ, tK, tV = (_t(torch, X, tdt) for X in (Q, K, V))
    O, LSE = autograd.attention_fused(plan, tQ, tK, tV, return_lse=True, backward="fused")
    assert O.dtype == torch.float32 and O.requires_grad and not LSE.requires_grad and tuple(LSE.shape) == (pat[0],)
    saved = O.grad_fn.saved_tensors
    assert len(saved) == 5 and not any(t.numel() == plan.nnz or plan.nnz in t.shape for t in saved)
    assert [t.data_ptr() for t in saved[:3]] == [t.data_ptr() for t in (tQ, tK, tV)]
    tdO = torch.from_numpy(dO).cuda()
    O.backward(tdO, retain_graph=True)
    torch.cuda.synchronize()
    grads = [t.grad.clone() for t in (tQ, tK, tV)]
    assert all(g.dtype == tdt for g in grads)
    failures = []
    for name, g, r, c in zip(("O", "dQ", "dK", "dV"), (O.detach(), *grads), ref, f32):
        top = np.abs(r).max()
        cpu_err = np.abs(c.astype(np.float64) - r).max() / top
        if dtype != F32 and name != "O":  # a gradient returned in fp16 carries that rounding too
            cpu_err = np.abs(half_values(c, dtype).astype(np.float64) - r).max() / top
        gpu_err = np.abs(g.float().cpu().numpy().astype(np.float64) - r).max() / top
        print(f"ATTENTION_FUSED_BWD {AC.DTYPE_NAME[dtype]} {name}: float32 CPU error {cpu_err:.3e}, GPU error "
              f"{gpu_err:.3e}, tolerance {8 * cpu_err:.3e}")
        assert cpu_err > 0
        if not gpu_err <= 8 * cpu_err:
            failures.append((name, gpu_err, 8 * cpu_err))
    assert not failures, failures
    O.backward(tdO)
    torch.cuda.synchronize()
    for name, g1, t in zip(("dQ", "dK", "dV"), grads, (tQ, tK, tV)):
        assert _same_bits(t.grad, g1 * 2), f"{name}: two backward passes do not accumulate"
    # the default path's forward gives the same O
    O2 = autograd.attention_fused(plan, tQ.detach(), tK.detach(), tV.detach())
    assert _same_bits(O2, O.detach())
    # only some inputs need a gradient: the same bits as the full call
    for need in ((True, False, False), (False, False, True), (False, True, True)):
        ts = [_t(torch, X, tdt, grad=n) for X, n in zip((Q, K, V), need)]
        autograd.attention_fused(plan, *ts, backward="fused").backward(tdO)
        torch.cuda.synchronize()
        for name, t, n, g in zip(("dQ", "dK", "dV"), ts, need, grads):
            assert (t.grad is None) == (not n), (need, name)
            assert not n or _same_bits(t.grad, g), f"needs_input_grad {need}: {name} differs from the full call"


def test_fused_backward_allocates_nothing_of_nnz_size():
    torch = torch_cuda()
    from bsmr import autograd
    n, d = 512, 16
    rp = (np.arange(n + 1) * n).astype(np.uint32)
    ci = np.tile(np.arange(n, dtype=np.uint32), n)
    plan = AC.make_plan((n, n, rp, ci))
    nnz_bytes = plan.nnz * 4
    assert nnz_bytes == 1 << 20
    X = [signed_data(n * d, 7 + i).reshape(n, d) for i in range(4)]
    grew = {}
    for mode in ("fused", "recompute"):
        for attempt in range(2):  # the first pass builds the plan's lists and warms the allocator
            ts = [_t(torch, x, torch.float32) for x in X[:3]]
            O = autograd.attention_fused(plan, *ts, backward=mode)
            tdO = torch.from_numpy(X[3]).cuda()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            O.backward(tdO)
            torch.cuda.synchronize()
            grew[mode] = torch.cuda.max_memory_allocated() - before
            del O, ts
        print(f"ATTENTION_FUSED_BWD memory: {mode} backward grows torch's peak by {grew[mode]} bytes "
              f"(nnz x 4 = {nnz_bytes})")
    assert grew["fused"] < nnz_bytes, grew
    assert grew["recompute"] > 3 * nnz_bytes, grew


def test_unknown_backward_raises_before_any_launch():
    torch = torch_cuda()
    from bsmr import autograd
    pat = AC.pattern("empty")
    plan = AC.make_plan(pat)
    z = functools.partial(torch.zeros, dtype=torch.float32, device="cuda")
    for bad in ("Fused", "", None, 1):
        with pytest.raises(ValueError, match="backward"):
            autograd.attention_fused(plan, z((pat[0], 32)), z((pat[1], 32)), z((pat[1], 32)), backward=bad)
    assert not plan.attention_prepared(32, 32) and not plan.attention_backward_prepared(32, 32)
