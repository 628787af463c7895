"""GPU: the fused sparse attention backward with its operands and gradients at and past 4 GiB
(tests/far_cases.py attention_far; D = Dv = 256 fp32 gives 1 KiB rows), after
tests/test_gpu_far_attention.py.

  bigN  96 x (2^22 + 64): K, V, GK and GV are 4 GiB + 64 KiB each
  bigM  (2^22 + 64) x 320: Q, O, GO and GQ are 4 GiB + 64 KiB each; the last row holds 300 entries, a
        split row: the row scratch, the reduce and GQ + dst D at the far end

Q, K, V, O and GO are NaN but for the used rows; the gradients start as NaN. Both exact sets must
come out bit for bit and signed data inside attention_bwd_cases.check_bound, all against the
compact reference; the destinations without an entry are counted on the device as exactly 0, nothing
of the full size is copied back. attention_backward_stats is what the list lengths give.
"""
import time

import numpy as np
import pytest

import attention_bwd_cases as BC
import far_cases as FC
from bsmr import F32, Plan
from gpu_util import torch_cuda
from sddmm_cases import FREE

pytestmark = pytest.mark.gpu
D = DV = 256


def backward_far_once(plan, far, inputs, scale):
    """dict(GQ, GK, GV) of the used rows / columns (numpy fp32) of one launch on full-shape device
    operands; every other destination is checked here to be exactly 0."""
    torch = torch_cuda()
    Q, K, V, O, GO, LSE = inputs
    dQ = FC.device_operand(far.M, far.rows, Q, F32)
    dK = FC.device_operand(far.N, far.cols, K, F32)
    dV = FC.device_operand(far.N, far.cols, V, F32)
    dO = FC.device_operand(far.M, far.rows, np.asarray(O, np.float32), F32)
    dGO = FC.device_operand(far.M, far.rows, np.asarray(GO, np.float32), F32)
    dL = FC.device_operand(far.M, far.rows, np.asarray(LSE, np.float32).reshape(-1, 1), F32)
    nan = lambda r, c: torch.full((r, c), float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
    gQ, gK, gV = nan(far.M, D), nan(far.N, D), nan(far.N, DV)
    plan.attention_backward(dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), dO.data_ptr(), dGO.data_ptr(), dL.data_ptr(),
                            D, DV, gQ.data_ptr(), gK.data_ptr(), gV.data_ptr(), scale,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del dQ, dK, dV, dO, dGO
    out = {}
    for k, t, used in (("GQ", gQ, far.rows), ("GK", gK, far.cols), ("GV", gV, far.cols)):
        out[k], stray = FC.take_rows(t, used)
        assert stray == 0, f"{stray} non-zero elements of {k} in destinations without an entry"
    return out


@pytest.mark.parametrize("name", ["bigN", "bigM"])
def test_far_attention_backward(name):
    far = FC.attention_far(name)
    pat = far.compact
    t0 = time.perf_counter()
    plan = Plan(far.M, far.N, far.rowptr, far.colidx, alpha=0.3, delta=0.3, free_mem_bytes=FREE)
    print(f"TIME attention_bwd_{name} plan {time.perf_counter() - t0:.2f}")
    what = f"far {name} f32 {D}x{DV}"
    t = time.perf_counter()
    Q, K, V, O, GO, LSE, winner = BC.selector_inputs(pat, D, DV, "random", 0.125)
    got = backward_far_once(plan, far, (Q, K, V, O, GO, LSE), 0.125)
    for k, w in zip(BC.OUTPUTS, BC.selector_expected(pat, GO, winner, D, DV)):
        BC.check_exact(got[k], w, f"{what} selector {k}")
    inputs = BC.flat_inputs(pat, D, DV)
    BC.check_exact_all(backward_far_once(plan, far, inputs, 0.125), BC.backward_ref(pat, *inputs, 0.125), f"{what} flat")
    Q, K, V, O, GO, LSE, opscale, _ = BC.signed_inputs(pat, D, DV, "wide", 0.25)
    got = backward_far_once(plan, far, (Q, K, V, O, GO, LSE), 0.25)
    BC.check_bound(got, BC.backward_ref(pat, Q, K, V, O, GO, LSE, 0.25), what, opscale)
    torch_cuda().cuda.empty_cache()
    print(f"TIME attention_bwd_{name} f32_{D}x{DV} {time.perf_counter() - t:.2f}")
    want = BC.expected_stats(FC.full_pattern(far), D, DV)
    assert plan.attention_backward_stats() == want, (plan.attention_backward_stats(), want)
    if name == "bigM":
        assert want["row_split"] >= 1 and want["row_max"] == 300
