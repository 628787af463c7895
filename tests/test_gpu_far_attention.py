"""GPU: the fused sparse attention with K, V, Q and O at and past 4 GiB (tests/far_cases.py
ATTN_RUNS; D = Dv = 256 fp32 gives 1 KiB rows).

  bigN  96 x (2^22 + 64): K and V are 4 GiB + 64 KiB each; a further run in bf16 with D 512 and
        Dv 256 (K 4 GiB, V 2 GiB)
  bigM  (2^22 + 64) x 320: Q and O are 4 GiB + 64 KiB each; the last row holds 300 entries, a split
        row: the scratch, k_attention_reduce and O + dst Dv at the far end

Q, K and V are NaN but for the used rows; O and LSE start as NaN. Selector data must give O and LSE
bit for bit, signed data stay inside attention_cases.check_bound, both against the compact
reference; the rows without an entry are counted on the device: O == 0 and LSE == -inf, nothing of
the full size is copied back. attention_stats is what the row lengths give.
"""
import time

import numpy as np
import pytest

import attention_cases as AC
import far_cases as FC
import spmm_cases as SP
from bsmr import Plan
from gpu_util import torch_cuda
from sddmm_cases import FREE

pytestmark = pytest.mark.gpu


def _expected_stats(pat):
    e = SP.expected_stats(pat, 1, AC.limits()["chunk"])
    return dict(segments=e["segments"], split_rows=e["split_dsts"], partials=e["partials"], max_row=e["max_list"],
                chunk=e["chunk"])


def attention_far_once(plan, far, Q, K, V, scale, dtype):
    """(O, LSE) of the used rows (numpy fp32) of one launch on full-shape device operands; the other
    rows are checked here: O exactly 0, LSE exactly -inf."""
    torch = torch_cuda()
    D, Dv = Q.shape[1], V.shape[1]
    dQ = FC.device_operand(far.M, far.rows, Q, dtype)
    dK = FC.device_operand(far.N, far.cols, K, dtype)
    dV = FC.device_operand(far.N, far.cols, V, dtype)
    dO = torch.full((far.M, Dv), float("nan"), dtype=torch.float32, device="cuda")
    dL = torch.full((far.M, 1), float("nan"), dtype=torch.float32, device="cuda")
    plan.attention(dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D, Dv, dO.data_ptr(), dL.data_ptr(), scale,
                   stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    del dQ, dK, dV
    O, stray = FC.take_rows(dO, far.rows)
    assert stray == 0, f"{stray} non-zero elements of O in rows without an entry"
    idx = torch.from_numpy(np.array(far.rows, np.int64)).cuda()
    LSE = dL.index_select(0, idx).cpu().numpy().ravel()
    dL.index_fill_(0, idx, float("-inf"))
    wrong = int(torch.count_nonzero(dL != float("-inf")))
    assert wrong == 0, f"LSE of {wrong} rows without an entry is not -inf"
    return O, LSE


@pytest.mark.parametrize("name", sorted(FC.ATTN_RUNS))
def test_far_attention(name):
    far = FC.attention_far(name)
    pat = far.compact
    t0 = time.perf_counter()
    plan = Plan(far.M, far.N, far.rowptr, far.colidx, alpha=0.3, delta=0.3, free_mem_bytes=FREE)
    print(f"TIME attention_{name} plan {time.perf_counter() - t0:.2f}")
    ok, msg = plan.check(0, verbose=False)
    assert ok, msg
    for D, Dv, dtype, _ in FC.ATTN_RUNS[name]:
        what = f"far {name} {AC.DTYPE_NAME[dtype]} {D}x{Dv}"
        t = time.perf_counter()
        for order in ("random", "ascending"):
            Q, K, V, winner, pi, base = AC.selector(pat, D, Dv, order, dtype)
            O, LSE = attention_far_once(plan, far, Q, K, V, 0.125, dtype)
            wantO, wantL = AC.selector_expected(V, winner, pi, base, 0.125, dtype)
            AC.check_exact(O, wantO, f"{what} O ({order})")
            AC.check_exact(LSE, wantL, f"{what} LSE ({order})")
        Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, "wide", 0.25)
        O, LSE = attention_far_once(plan, far, Q, K, V, 0.25, dtype)
        AC.check_bound(O, LSE, AC.attention_ref(pat, Q, K, V, 0.25, dtype), what, opscale)
        torch_cuda().cuda.empty_cache()
        print(f"TIME attention_{name} {AC.DTYPE_NAME[dtype]}_{D}x{Dv} {time.perf_counter() - t:.2f}")
    want = _expected_stats(FC.full_pattern(far))
    assert plan.attention_stats() == want, (plan.attention_stats(), want)
    if name == "bigM":
        assert want["split_rows"] >= 1 and want["max_row"] == 300
