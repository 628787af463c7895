"""GPU: every k_spmm instantiation (bsmr_spmm / bsmr_spmm_t) against the float64 reference, exact
and bounded (reference, data, bound, case table: tests/spmm_cases.py).

* every SPMM_CASES row (the 15 fixed instantiations, the generic form at every lane count L = 2 ..
  64 and at 1, 2, 3 and 4 column tiles) on `staircase` (both sides see every list length 0 .. 271,
  so every segment count 0 .. chunk against the lane groups, the unroll and the 64-entry batch),
  both sides, default chunk and chunk 32;
* one fixed and one generic case per dtype on `hub` (a list of 2048: 32 batches, 16 or 64 partial
  rows) and `zipf_shuffled` (columns of a CSR row in file order);
* a fixed (512 B fp32) and a generic (96 B bf16) case on `staircase` and `hub` at chunk 1 (every
  entry a partial row), 64, 65 and 1 << 20 (no destination split: the hub row is one segment).

Every launch: grid data gives Y == ref bit for bit; signed data stays within signed_bound_tight
(printed as "RATIO spmm/<case> <value>"; DESIGN.md section 11.2 records the worst); Y starts as
NaN and ends finite; empty destinations are exactly 0; Plan.spmm_stats equals the counts numpy
derives from the list lengths.
"""
import functools

import numpy as np
import pytest

from bsmr import BF16, F16, F32, Plan
from gpu_util import spmm_device, to_device, torch_cuda
from sddmm_cases import as_seen, grid_data, signed_data
from spmm_cases import (DEFAULT_CHUNK, SPMM_CASES, assert_exact, assert_tight, case_id, expected_stats, grid_values,
                        pattern, signed_values, spmm_form, spmm_ref)

pytestmark = pytest.mark.gpu

FREE = 288 * 1024 ** 3


def plan_of(name):
    M, N, rp, ci = pattern(name)
    return Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE)


@functools.lru_cache(maxsize=6)
def _operands(name, K, dtype, data):
    pat = pattern(name)
    M, N, _, ci = pat
    gen, vals = (grid_data, grid_values) if data == "grid" else (signed_data, signed_values)
    A = as_seen(gen(M * K, 101), dtype).reshape(M, K)
    B = as_seen(gen(N * K, 202), dtype).reshape(N, K)
    V = vals(len(ci), 303)
    out = (A, B, V, spmm_ref(pat, 1, V, B), spmm_ref(pat, 2, V, A))
    for x in (A, B, V) + out[3] + out[4]:
        x.setflags(write=False)
    return out


def operands(name, K, dtype, data):
    """(A, B, V, ref of side 1, ref of side 2): operands as the kernel sees them and their float64
    references, read-only, computed once per (pattern, K, dtype) and shared by the chunk variants.
    Grid data is the same in every dtype."""
    return _operands(name, K, F32 if data == "grid" else dtype, data)


def check_case(name, K, dtype, chunks):
    torch_cuda()
    pat = pattern(name)
    plan = plan_of(name)
    cid = case_id(K, dtype)
    for data in ("grid", "signed"):
        A, B, V, ref1, ref2 = operands(name, K, dtype, data)
        dA, dB, dV = to_device(A, dtype), to_device(B, dtype), to_device(V, F32)
        for chunk in chunks:
            plan.prepare_spmm(K, 3, chunk=chunk)
            assert plan.spmm_prepared(K, 3)
            for side, dX, ref in ((1, dB, ref1), (2, dA, ref2)):
                assert plan.spmm_stats(side) == expected_stats(pat, side, chunk), (name, side, chunk)
                Y = spmm_device(plan, side, dV, dX, K, dtype)
                what = f"{name} {cid} chunk {chunk} side {side} {data}"
                if data == "grid":
                    assert_exact(Y, ref, what)
                else:
                    assert_tight(Y, ref, what, cid)


@pytest.mark.parametrize("K,dtype", SPMM_CASES, ids=[case_id(*kd) for kd in SPMM_CASES])
def test_every_instantiation_on_the_staircase(K, dtype):
    check_case("staircase", K, dtype, (DEFAULT_CHUNK, 32))


# one fixed and one generic instantiation per dtype: 512 B and 384 B (24 of 32 lanes) fp32; the
# two-chunk 2 KiB row in both half types; two column tiles fp16; 96 B (6 of 8 lanes) bf16
HUB_CASES = [(128, F32), (96, F32), (1024, F16), (640, F16), (1024, BF16), (48, BF16)]


@pytest.mark.parametrize("K,dtype", HUB_CASES, ids=[case_id(*kd) for kd in HUB_CASES])
@pytest.mark.parametrize("name", ["hub", "zipf_shuffled"])
def test_hub_and_file_order(name, K, dtype):
    assert (K, dtype) in SPMM_CASES
    check_case(name, K, dtype, (DEFAULT_CHUNK, 32))


def test_hub_cases_take_a_fixed_and_a_generic_form_per_dtype():
    for dtype in (F32, F16, BF16):
        assert {spmm_form(K, d)["fixed"] for K, d in HUB_CASES if d == dtype} == {True, False}


@pytest.mark.parametrize("chunk", [1, 64, 65, 1 << 20])
@pytest.mark.parametrize("K,dtype", [(128, F32), (48, BF16)], ids=["K128_f32", "K48_bf16"])
@pytest.mark.parametrize("name", ["staircase", "hub"])
def test_chunks(name, K, dtype, chunk):
    if chunk == 1 << 20:
        for side in (1, 2):
            st = expected_stats(pattern(name), side, chunk)
            assert st["split_dsts"] == 0 and st["partials"] == 0
            if name == "hub" and side == 1:
                assert st["max_list"] == 2048 and st["segments"] == 67  # the hub row is one segment
    check_case(name, K, dtype, (chunk,))
