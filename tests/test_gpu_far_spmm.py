"""GPU: the plan-based SpMM with X and Y at and past 4 GiB (tests/far_cases.py SPMM_RUNS).

  bigN  96 x (2^21 + 64): side 1 gathers X = B (4 GiB + 128 KiB at 2 KiB rows: fp32 K 512 and bf16
        K 1024), side 2 writes Y of that size
  bigM  (2^21 + 64) x 192, the last row a hub of all 192 columns (the pattern has no more): side 1
        writes Y past 4 GiB, side 2 gathers X = A (fp32 K 512 and bf16 K 1024)

Both plans are prepared with chunk 32, so the hubs and the band rows (about 38 entries) are split
destinations: k_spmm's partial rows and k_spmm_reduce store at the far end too. X is NaN but for
the used rows; Y starts as NaN. On the device the used destinations are compared with the compact
float64 reference (bit for bit on grid values, spmm_cases.assert_tight on signed values) and every
other row is counted: no non-zero element, without copying Y back.
"""
import time

import numpy as np
import pytest

import far_cases as FC
import spmm_cases as SP
from bsmr import Plan
from gpu_util import spmm_launch, torch_cuda
from sddmm_cases import FREE

pytestmark = pytest.mark.gpu
KMAX = 1024


@pytest.mark.parametrize("name", sorted(FC.SPMM_RUNS))
def test_far_spmm(name):
    torch = torch_cuda()
    far = FC.spmm_far(name)
    t0 = time.perf_counter()
    plan = Plan(far.M, far.N, far.rowptr, far.colidx, alpha=0.3, delta=0.3, free_mem_bytes=FREE)
    t1 = time.perf_counter()
    plan.prepare_spmm(KMAX, 3, FC.SPMM_CHUNK)
    t2 = time.perf_counter()
    print(f"TIME spmm_{name} plan {t1 - t0:.2f}")
    print(f"TIME spmm_{name} prepare {t2 - t1:.2f}")
    for side in (1, 2):
        want = SP.expected_stats(FC.full_pattern(far), side, FC.SPMM_CHUNK)
        assert plan.spmm_stats(side) == want, (side, plan.spmm_stats(side), want)
        assert want["split_dsts"] > 0 and want["max_list"] > FC.SPMM_CHUNK
    ok, msg = plan.check(0, verbose=False)
    assert ok, msg
    for side, K, dtype, _ in FC.SPMM_RUNS[name]:
        dst, src, nd, ns = FC.spmm_used(far, side)
        what = f"far {name} side {side} K {K} {SP.DTYPE_NAME[dtype]}"
        t = time.perf_counter()
        for data in ("grid", "signed"):
            V, Xc, ref = FC.compact_spmm(far, side, K, dtype, data)
            dX = FC.device_operand(ns, src, Xc, dtype)
            dV = torch.from_numpy(V).cuda()
            dY = torch.full((nd, K), float("nan"), dtype=torch.float32, device="cuda")
            spmm_launch(plan, side, dV, dX, K, dtype, dY)
            torch.cuda.synchronize()
            got, stray = FC.take_rows(dY, dst)
            del dX, dY
            assert stray == 0, f"{what}: {stray} non-zero elements in rows without an entry"
            if data == "grid":
                SP.assert_exact(got, ref, what)
            else:
                SP.assert_tight(got, ref, what, "far")
        torch.cuda.empty_cache()
        print(f"TIME spmm_{name} side{side}_K{K}_{SP.DTYPE_NAME[dtype]} {time.perf_counter() - t:.2f}")
