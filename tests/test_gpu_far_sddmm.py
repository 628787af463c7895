"""GPU: every SDDMM launch where 32-bit byte offsets and the packed 22-bit fields run out
(tests/far_cases.py; tests/test_far_cases_cpu.py shows, without a GPU, that each shape crosses the
boundary it names and that the reference would notice).

Per case: the operands are device tensors of the full shape, NaN but for the used rows; P starts as
NaN and must end finite; grid data must equal the compact float64 reference bit for bit
(sddmm_cases.assert_exact), signed data stay inside sddmm_cases.sddmm_bound; bsmr_plan_check passes;
the launch kind and slot are the library's own account (gpu_util.plan_launch) and Plan.stats().

  rb_B_below_4G    96 x (2^21 - 1), fp32 K 512: row-block slot 4, B byte offsets up to 2^32 - 2 KiB;
                   again with tile_min_f32 = 0 (the dense block in the last 16 columns a kept tile)
  rb_B_1k          96 x (2^22 - 1), bf16 K 512 and fp32 K 256: slot 3, column field 2^22 - 2
  rb_col_all_ones  96 x 2^22, fp32 K 128 and fp16 K 256: slot 2, a piece word 0x03FFFFFF (column
                   2^22 - 1, 16 entries; layout rowblock and full bands, far_cases.py says why);
                   also out_staged = 1 and out_packed = 0
  cm_B_at_4G       96 x 2^21, fp32 K 512: the first shape past the row-block rule, column-major
  cm_B_past_4G     96 x (2^21 + 64), fp32 K 512 and fp16 K 1024: column-major / half, tile and residual
  cm_N_past_2p22   96 x (2^22 + 1), fp32 K 16 and bf16 K 32: the column no 22-bit field holds
  rb_A_past_4G     (2^21 + 64) x 192, fp32 K 512 and bf16 K 1024: slot 4 with A past 4 GiB; layout
                   colmajor; bsmr_sddmm_panels over three ranges, bsmr_sddmm_panels_local on the last;
                   col_blocks = 1 on this plan is skipped (launch_select.cpp col_block_candidate):
                   the rb_col_blocks bit stays clear and P is exact
  cols_A_below_4G  (2^21 - 1) x 192, col_blocks = 1: legal, the bit is set, A offsets up to 2^32 - 2 KiB
  batch_past_4G    2^15 x 2^15, fp32 K 512, 65 batches: the batch strides pass 4 GiB

  packed_nnz_2p22  4096 x 4096 with exactly 2^22 and 2^22 + 1 entries, fp32 K 32, layout rowblock,
                   out_staged = 0: packed output with the position field all ones, unpacked one past
  far_dense / far_ptile  128 x (2^21 + 128), bf16 K 512: the dense-sampled launch (dense_min lowered)
                   and the panel-tile launch (a 16 x 16 block mask, ptile = 1) with B past 2 GiB

Every test prints "TIME <case> <stage> <seconds>" (DESIGN.md "Address widths" records them).
"""
import ctypes as C
import time

import numpy as np
import pytest

import bsmr
import far_cases as FC
import sddmm_cases as SD
from bsmr import BF16, F16, F32, Plan, synth
from gpu_util import nan_output, plan_launch, torch_cuda

pytestmark = pytest.mark.gpu
FREE = SD.FREE


class Clock:
    def __init__(self, case):
        self.case, self.t = case, time.perf_counter()

    def lap(self, stage):
        torch_cuda().cuda.synchronize()
        now = time.perf_counter()
        print(f"TIME {self.case} {stage} {now - self.t:.2f}")
        self.t = now


def make_plan(far, layout="auto", tuning=None):
    return Plan(far.M, far.N, far.rowptr, far.colidx, alpha=0.3, delta=0.3, free_mem_bytes=FREE, layout=layout,
                tuning=tuning or {})


def launch(plan, dA, dB, K, dtype, nnz):
    torch = torch_cuda()
    dP = nan_output(nnz)
    plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), stream=torch.cuda.current_stream().cuda_stream,
               dtype=dtype)
    torch.cuda.synchronize()
    return dP.cpu().numpy()[:nnz]


def evidence(plan, K, dtype, kind, slot=-1, col_blocks=False, tiles=None):
    got = plan_launch(plan, K, dtype)
    st = plan.stats()
    assert (got["kind"], got["slot"]) == (kind, slot), (got, st)
    if kind == "rowblock":
        assert [i for i, n in enumerate(st["rb_items"]) if n] == [slot], st
        assert bool(st["rb_col_blocks"] & (1 << slot)) == col_blocks, st
        if tiles is not None:
            assert (st["rb_tiles"][slot] > 0) == tiles, st
    else:
        assert not any(st["rb_items"]), st
    ok, msg = plan.check(K, dtype, verbose=False)
    assert ok, msg
    return st


def run_case(name, plan, K, dtype, kind, slot=-1, clock=None, **proof):
    """Both data sets through one launch each on `plan`; the evidence after the first."""
    far = FC.sddmm_far(name)
    nnz = len(far.colidx)
    what = f"{name} K {K} {SD.DTYPE_NAME[dtype]}"
    for data in ("grid", "signed"):
        Ac, Bc, P, S = FC.sddmm_reference(name, K, dtype, data)
        dA = FC.device_operand(far.M, far.rows, Ac, dtype)
        dB = FC.device_operand(far.N, far.cols, Bc, dtype)
        got = launch(plan, dA, dB, K, dtype, nnz)
        del dA, dB
        if data == "grid":
            SD.assert_exact(got, P, what)
            evidence(plan, K, dtype, kind, slot, **proof)
        else:
            SD.assert_bound(got, P, S, K, what, "far/" + kind)
    torch_cuda().cuda.empty_cache()
    if clock:
        clock.lap(f"K{K}_{SD.DTYPE_NAME[dtype]}")


def rb_piece_words(plan, K, dtype):
    """The second word (column | (length - 1) << 22) of every piece of the whole-plan row-block
    layout (the debug export bsmr_debug_rb_pieces)."""
    f = bsmr.lib().bsmr_debug_rb_pieces
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    n = C.c_uint64()
    assert f(plan.h, K, dtype, None, C.byref(n)) == 0
    buf = np.zeros(n.value, np.uint32)
    assert f(plan.h, K, dtype, buf.ctypes.data, C.byref(n)) == 0
    items, pieces = int(buf[0]), int(buf[1])
    return buf[2 + 5 * items:2 + 5 * items + 2 * pieces].reshape(pieces, 2)[:, 1]


def test_rb_B_below_4G():
    name, clock = "rb_B_below_4G", Clock("rb_B_below_4G")
    far = FC.sddmm_far(name)
    plan = make_plan(far)
    clock.lap("plan")
    assert plan.stats()["num_dense_tiles"] > 0
    run_case(name, plan, 512, F32, "rowblock", 4, clock, tiles=False)
    del plan
    plan = make_plan(far, tuning={"tile_min_f32": 0})  # the dense block at the last columns on MFMA
    run_case(name, plan, 512, F32, "rowblock", 4, clock, tiles=True)


def test_rb_B_1k():
    name, clock = "rb_B_1k", Clock("rb_B_1k")
    plan = make_plan(FC.sddmm_far(name))
    clock.lap("plan")
    run_case(name, plan, 512, BF16, "rowblock", 3, clock)
    del plan
    plan = make_plan(FC.sddmm_far(name))  # (one row size per plan: evidence() reads rb_items)
    run_case(name, plan, 256, F32, "rowblock", 3, clock)


@pytest.mark.parametrize("tuning", [{}, {"out_staged": 1}, {"out_packed": 0}], ids=["default", "staged", "unpacked"])
def test_rb_col_all_ones(tuning):
    name, clock = "rb_col_all_ones", Clock("rb_col_all_ones")
    far = FC.sddmm_far(name)
    plan = make_plan(far, layout="rowblock", tuning=tuning)
    clock.lap("plan")
    run_case(name, plan, 128, F32, "rowblock", 2, clock)
    words = rb_piece_words(plan, 128, F32)
    assert (words == 0x03FFFFFF).any(), "no piece of 16 entries in column 2^22 - 1"
    del plan
    plan = make_plan(far, layout="rowblock", tuning=tuning)
    run_case(name, plan, 256, F16, "rowblock", 2, clock)


def test_cm_B_at_4G():
    name, clock = "cm_B_at_4G", Clock("cm_B_at_4G")
    plan = make_plan(FC.sddmm_far(name))
    clock.lap("plan")
    run_case(name, plan, 512, F32, "colmajor", -1, clock)


def test_cm_B_past_4G():
    name, clock = "cm_B_past_4G", Clock("cm_B_past_4G")
    plan = make_plan(FC.sddmm_far(name))
    clock.lap("plan")
    st = plan.stats()
    assert st["num_dense_tiles"] > 0 and st["num_residual"] > 0  # the tile kernel and the residual
    run_case(name, plan, 512, F32, "colmajor", -1, clock)
    run_case(name, plan, 1024, F16, "half", -1, clock)


def test_cm_N_past_2p22():
    name, clock = "cm_N_past_2p22", Clock("cm_N_past_2p22")
    plan = make_plan(FC.sddmm_far(name))
    clock.lap("plan")
    run_case(name, plan, 16, F32, "colmajor", -1, clock)
    run_case(name, plan, 32, BF16, "half", -1, clock)


def test_rb_A_past_4G():
    name, clock = "rb_A_past_4G", Clock("rb_A_past_4G")
    far = FC.sddmm_far(name)
    plan = make_plan(far)
    clock.lap("plan")
    run_case(name, plan, 512, F32, "rowblock", 4, clock)
    del plan
    plan = make_plan(far)
    run_case(name, plan, 1024, BF16, "rowblock", 4, clock)
    del plan
    plan = make_plan(far, layout="colmajor")
    run_case(name, plan, 512, F32, "colmajor", -1, clock)
    run_case(name, plan, 1024, BF16, "half", -1, clock)


def test_rb_A_past_4G_panels():
    """bsmr_sddmm_panels over three ranges writes every entry once; bsmr_sddmm_panels_local on the
    last range, from that range's own A rows, writes exactly its rows' entries."""
    torch = torch_cuda()
    name, K, clock = "rb_A_past_4G", 512, Clock("rb_A_past_4G_panels")
    far = FC.sddmm_far(name)
    nnz = len(far.colidx)
    plan = make_plan(far)
    Ac, Bc, P, _ = FC.sddmm_reference(name, K, F32, "grid")
    dA = FC.device_operand(far.M, far.rows, Ac, F32)
    dB = FC.device_operand(far.N, far.cols, Bc, F32)
    s = torch.cuda.current_stream().cuda_stream
    shards = [plan.shard(K, r, 3) for r in range(3)]
    assert shards[0][0] == 0 and shards[-1][1] == plan.stats()["num_row_panels"]
    assert all(p0 < p1 for p0, p1 in shards), shards
    dP = nan_output(nnz)
    for p0, p1 in shards:
        plan.sddmm_panels(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), p0, p1, stream=s)
    torch.cuda.synchronize()
    SD.assert_exact(dP.cpu().numpy()[:nnz], P, name + " panels")
    assert plan_launch(plan, K, F32)["slot"] == 4
    p0, p1 = shards[-1]
    order = plan.array("reorderedRows").astype(np.int64)
    local = order[16 * p0:min(16 * p1, len(order))]
    assert local.max() >= 1 << 21  # the far rows are in the range
    dAl = dA.index_select(0, torch.from_numpy(local).cuda())
    dP = nan_output(nnz)
    plan.sddmm_panels_local(dAl.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), p0, p1, stream=s)
    torch.cuda.synchronize()
    got = dP.cpu().numpy()[:nnz]
    mine = np.isin(far.rows[np.repeat(np.arange(far.compact[0]), np.diff(far.compact[2].astype(np.int64)))], local)
    assert mine.any() and not mine.all()
    SD.assert_exact(got[mine], P[mine], name + " panels_local")
    assert np.isnan(got[~mine]).all(), "bsmr_sddmm_panels_local wrote outside its rows"
    evidence(plan, K, F32, "rowblock", 4)
    clock.lap("all")


def test_cols_A_past_4G_falls_back_to_row_blocks():
    """col_blocks = 1 with A past 4 GiB: the column-block launch would gather A rows with a 32-bit
    byte offset (rows from 2^21 on would read rows 0 .. 63), so the candidate is skipped: the bit
    stays clear, no error, P exact."""
    name, clock = "rb_A_past_4G", Clock("cols_A_past_4G")
    plan = make_plan(FC.sddmm_far(name), tuning={"col_blocks": 1})
    clock.lap("plan")
    run_case(name, plan, 512, F32, "rowblock", 4, clock, col_blocks=False)
    assert plan.stats()["rb_col_blocks"] == 0


def test_cols_A_below_4G_runs_column_blocks():
    name, clock = "cols_A_below_4G", Clock("cols_A_below_4G")
    plan = make_plan(FC.sddmm_far(name), tuning={"col_blocks": 1})
    clock.lap("plan")
    run_case(name, plan, 512, F32, "rowblock", 4, clock, col_blocks=True)


def test_batch_past_4G():
    """65 batches of a 2^15 x 2^15 plan at 2 KiB rows: batch b's operands start b x 64 MiB in, past
    4 GiB from batch 64 on. Batch b is the base operands times 2^-(b mod 3), so P_b = 4^-(b mod 3)
    P_0 exactly on grid data."""
    torch = torch_cuda()
    clock = Clock("batch_past_4G")
    M = N = 1 << 15
    K, NB = 512, 65
    counts = np.zeros(M, np.int64)
    counts[::16] = 4
    pat = synth.random_rows(M, N, counts, seed=17, zipf=1.1)
    nnz = len(pat[3])
    assert 0 < nnz < 10 ** 4
    A, B = SD.grid_data(M * K, 301).reshape(M, K), SD.grid_data(N * K, 302).reshape(N, K)
    P0, _ = SD.sddmm_ref(pat, A, B)
    plan = Plan(M, N, pat[2], pat[3], alpha=0.3, delta=0.3, free_mem_bytes=FREE)
    clock.lap("plan")
    scale = torch.tensor([2.0 ** -(b % 3) for b in range(NB)], device="cuda").reshape(NB, 1, 1)
    dA = torch.from_numpy(A).cuda().unsqueeze(0) * scale
    dB = torch.from_numpy(B).cuda().unsqueeze(0) * scale
    assert dA.is_contiguous() and dA.numel() * 4 > 1 << 32
    dP = torch.full((NB, nnz), float("nan"), dtype=torch.float32, device="cuda")
    plan.sddmm_batch(NB, dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = dP.cpu().numpy()
    assert np.isfinite(got).all()
    for b in (0, 32, 33, 64):
        SD.assert_exact(got[b], P0 * 4.0 ** -(b % 3), f"batch_past_4G batch {b}")
    evidence(plan, K, F32, "rowblock", 4)
    clock.lap("run")


def _half_launch(kind, tuning, want):
    name, K, clock = f"far_{kind}", 512, Clock(f"far_{kind}")
    far = FC.half_launch_far(kind)
    nnz = len(far.colidx)
    plan = make_plan(far, tuning=tuning)
    clock.lap("plan")
    for data in ("grid", "signed"):
        Ac, Bc, P, S = FC.compact_sddmm(far, K, BF16, data)
        got = launch(plan, FC.device_operand(far.M, far.rows, Ac, BF16), FC.device_operand(far.N, far.cols, Bc, BF16),
                     K, BF16, nnz)
        if data == "grid":
            SD.assert_exact(got, P, name)
        else:
            SD.assert_bound(got, P, S, K, name, "far/" + kind)
    st = plan.stats()
    assert plan_launch(plan, K, BF16)["kind"] == want, (plan_launch(plan, K, BF16), st)
    ok, msg = plan.check(K, BF16, verbose=False)
    assert ok, msg
    clock.lap("run")
    return st


def test_dense_sampled_at_a_far_shape():
    """128 x (2^21 + 128), bf16 K 512: dense_min lowered to 10^-6 (the pattern holds about 10^-5 of
    M N) so that the dense-sampled launch is chosen; its 128 x 128 tiles stage whole B tiles past
    2 GiB, NaN rows included, and sample only the stored entries."""
    st = _half_launch("dense", {"dense_min": 1e-6}, "dense")
    assert st["dense_sampled_tiles"] > 0 and st["ptile_items"] == 0 and not any(st["rb_items"])


def test_panel_tile_at_a_far_shape():
    """The same shape with a 16 x 16 block mask in the far column bands, ptile = 1."""
    st = _half_launch("ptile", {"ptile": 1}, "ptile")
    assert st["ptile_items"] > 0 and st["num_dense_tiles"] > 0 and st["dense_sampled_tiles"] == 0


@pytest.mark.parametrize("extra", [0, 1], ids=["nnz_2p22", "nnz_2p22_plus_1"])
def test_packed_nnz_2p22(extra):
    """4096 x 4096 with exactly 2^22 (and one more) stored entries, fp32 K 32, layout rowblock,
    out_staged = 0: the packed output keeps the CSR position in the metadata's 22 bits, up to all
    ones at 2^22 entries; one entry more and the layout is unpacked. P is exact either way and
    bit-identical to out_packed = 0, and bsmr_plan_check passes on all four plans."""
    torch = torch_cuda()
    clock = Clock("packed_nnz_2p22" + ("_plus_1" if extra else ""))
    M = N = 4096
    K, nnz = 32, (1 << 22) + extra
    keep = np.zeros(M * N, bool)
    keep[np.random.default_rng(23).permutation(M * N)[:nnz]] = True
    keep = keep.reshape(M, N)
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint32)
    ci = np.nonzero(keep)[1].astype(np.uint32)
    assert len(ci) == nnz
    A, B = SD.grid_data(M * K, 401).reshape(M, K), SD.grid_data(N * K, 402).reshape(N, K)
    P, _ = SD.sddmm_ref((M, N, rp, ci), A, B)
    clock.lap("reference")
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    out = {}
    for packed in (-1, 0):
        plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, layout="rowblock",
                    tuning={"out_staged": 0, "out_packed": packed})
        clock.lap(f"plan_packed{packed}")
        out[packed] = launch(plan, dA, dB, K, F32, nnz)
        SD.assert_exact(out[packed], P, f"packed_nnz_2p22 + {extra} out_packed {packed}")
        clock.lap(f"run_packed{packed}")
        # the launch, Plan.stats() and bsmr_plan_check, whose packed branch reads the position from
        # the metadata's low 22 bits: all ones at 2^22 entries, the `out` array one entry past
        st = evidence(plan, K, F32, "rowblock", 0, tiles=False)
        assert st["nnz"] == nnz and st["rb_entries"][0] == nnz, st
        assert plan_launch(plan, K, F32)["packed"] == (packed != 0 and extra == 0)
        clock.lap(f"check_packed{packed}")
        del plan
    assert np.array_equal(out[-1].view(np.uint32), out[0].view(np.uint32))
