"""GPU: every forward SDDMM launch path against a float64 reference on signed data.

tests/sddmm_cases.py holds the reference (numpy float64 from the CSR, on the operands as the kernel
sees them), the two data sets, the bound and the table CASES of kernel instantiations with the
plan options that reach each and the Plan.stats() evidence that it ran. Per case:

  * grid data (multiples of 1/8 in [-4, 4): every partial sum is exact in fp32 in any order):
    P == reference bit for bit;
  * signed data (uniform [-1, 1), full mantissa): |P - ref| <= min(2 K, 8 sqrt K) 2^-24 sum|a b|
    + 1e-6, derived in sddmm_cases and not tuned; the worst ratio is printed ("RATIO kind x case");
  * the stats evidence of the case, so a silent fall-back to another launch fails;
  * P starts as NaN and ends finite everywhere.

The same two checks through the other ways into a kernel: bsmr_sddmm_batch (three batches of
different data, grid.y and the batch strides), bsmr_sddmm_panels over three uneven panel ranges
(each range writes exactly its rows' entries), bsmr_sddmm_panels_local, and a graph-captured first
launch after Plan.prepare replayed with the operands changed in place.
"""
import numpy as np
import pytest

import bsmr
from bsmr import Plan
from gpu_util import nan_output, path_evidence, plan_launch, rb_store, sddmm_once, to_device, torch_cuda
from sddmm_cases import (BY_NAME, CASES, ONE_PER_KIND, PANEL_CASES, assert_bound, assert_exact, pattern,
                         plan_kwargs, rb_slot, reference)
from spmm_cases import entry_rows

pytestmark = pytest.mark.gpu

UNSUPPORTED = 6  # BSMR_ERR_UNSUPPORTED


def _plan(case):
    M, N, rp, ci = pattern(case.pattern)
    return Plan(M, N, rp, ci, **plan_kwargs(case))


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case_matches_float64(name):
    case = BY_NAME[name]
    nnz = len(pattern(case.pattern)[3])
    plan = _plan(case)
    A, B, ref, _ = reference(case.pattern, case.K, case.dtype, "grid")
    assert_exact(sddmm_once(plan, A, B, case.K, nnz, case.dtype), ref, name + " grid")
    A, B, ref, S = reference(case.pattern, case.K, case.dtype, "signed")
    assert_bound(sddmm_once(plan, A, B, case.K, nnz, case.dtype), ref, S, case.K, name, case.kind)
    assert not path_evidence(case, plan)


def _trace_words(plan):
    """The timeline of the plan's last traced launch (debug export bsmr_debug_trace, not in the
    header): 4 u64 per wave {start, mid, end, XCC id << 60 | tile end}."""
    import ctypes as C
    L = bsmr.lib()
    L.bsmr_debug_trace.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    n = C.c_uint64()
    assert L.bsmr_debug_trace(plan.h, None, C.byref(n)) == 0
    buf = np.zeros(n.value, np.uint64)
    assert L.bsmr_debug_trace(plan.h, buf.ctypes.data, C.byref(n)) == 0
    return buf


@pytest.mark.parametrize("name", ["rb_K256_bf16", "rb_staged_K128_f32"])
def test_full_form_timeline(name):
    """diag = 32 (the tools' timeline) on a case that keeps MFMA tiles and on a staged fp32 one: the
    launch is the full single-item form, P is still right, and the trace holds 4 words per wave of
    every item slot: 0 < start <= mid <= end for the waves of a real item, zeros (the launch clears
    the buffer, Plan::prepare_trace, and a padding item returns at once) for a padding one."""
    base = BY_NAME[name]
    case = base._replace(tuning=dict(base.tuning, diag=32))
    K, dtype, nnz = case.K, case.dtype, len(pattern(case.pattern)[3])
    plan = _plan(case)
    A, B, ref, _ = reference(case.pattern, K, dtype, "grid")
    assert_exact(sddmm_once(plan, A, B, K, nnz, dtype), ref, name + " traced grid")
    A, B, ref, S = reference(case.pattern, K, dtype, "signed")
    assert_bound(sddmm_once(plan, A, B, K, nnz, dtype), ref, S, K, name + " traced", case.kind + "/trace")
    assert not path_evidence(case, plan)
    launch = plan_launch(plan, K, dtype)
    assert launch["kind"] == "rowblock" and not launch["lite"] and not launch["pairs"], launch
    st, slot = plan.stats(), rb_slot(K, dtype)
    if name == "rb_K256_bf16":
        assert st["rb_tiles"][slot] > 0
    else:
        assert rb_store(plan, K, dtype, raw=False)["outLds"] > 0
    nw = launch["NT"] // 64
    words = _trace_words(plan)
    assert len(words) == 4 * st["rb_items"][slot] * nw
    t = words.reshape(-1, nw, 4)
    real = rb_store(plan, K, dtype, raw=False)["real"]
    assert len(real) == len(t) and real.any()
    t0, tm, t1 = (t[real][:, :, i] for i in range(3))
    assert (t0 > 0).all() and (t0 <= tm).all() and (tm <= t1).all()
    assert not t[~real].any()


@pytest.mark.parametrize("name", ONE_PER_KIND)
def test_batch_of_three(name):
    """bsmr_sddmm_batch: batch b reads A + b M K, B + b N K and writes P + b nnz."""
    torch = torch_cuda()
    case = BY_NAME[name]
    pat = pattern(case.pattern)
    M, N, _, ci = pat
    K, dtype, nnz, nb = case.K, case.dtype, len(ci), 3
    plan = _plan(case)
    for data in ("grid", "signed"):
        ops = [reference(case.pattern, K, dtype, data, seed=b) for b in range(nb)]
        dA = to_device(np.stack([o[0] for o in ops]), dtype)
        dB = to_device(np.stack([o[1] for o in ops]), dtype)
        dP = nan_output(nb * nnz)
        plan.sddmm_batch(nb, dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
                         stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
        torch.cuda.synchronize()
        P = dP.cpu().numpy().reshape(nb, nnz)
        for b, (_, _, ref, S) in enumerate(ops):
            if data == "grid":
                assert_exact(P[b], ref, f"{name} batch {b} grid")
            else:
                assert_bound(P[b], ref, S, K, f"{name} batch {b}", case.kind + "/batch")
    assert not path_evidence(case, plan)


def _uneven_ranges(npanels):
    """Three panel ranges of different sizes covering [0, npanels): one panel, about a third of
    the rest, the rest."""
    a = 1
    b = a + max(1, (npanels - 1) // 3)
    assert a < b < npanels
    return [(0, a), (a, b), (b, npanels)]


def _written_by(plan, pat, p0, p1):
    """Mask over the entries: those of the rows at reordered positions [16 p0, 16 p1)."""
    M, _, rp, _ = pat
    rows = plan.array("reorderedRows")[16 * p0:16 * p1]
    mine = np.zeros(M, bool)
    mine[rows] = True
    return mine[entry_rows(M, rp)]


@pytest.mark.parametrize("name", PANEL_CASES)
def test_panels_in_three_uneven_shards(name):
    torch = torch_cuda()
    case = BY_NAME[name]
    pat = pattern(case.pattern)
    K, dtype, nnz = case.K, case.dtype, len(pat[3])
    plan = _plan(case)
    s = torch.cuda.current_stream().cuda_stream
    ranges = _uneven_ranges(plan.stats()["num_row_panels"])
    for data in ("grid", "signed"):
        A, B, ref, S = reference(case.pattern, K, dtype, data)
        dA, dB, dP = to_device(A, dtype), to_device(B, dtype), nan_output(nnz)
        done = np.zeros(nnz, bool)
        for p0, p1 in ranges:
            plan.sddmm_panels(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), p0, p1, stream=s, dtype=dtype)
            torch.cuda.synchronize()
            done |= _written_by(plan, pat, p0, p1)
            assert np.array_equal(np.isfinite(dP.cpu().numpy()[:nnz]), done), \
                f"{name}: panels [{p0}, {p1}) did not write exactly their rows' entries"
        assert done.all()
        P = dP.cpu().numpy()[:nnz]
        if data == "grid":
            assert_exact(P, ref, name + " panels grid")
        else:
            assert_bound(P, ref, S, K, name + " panels", case.kind + "/panels")
    st = plan.stats()
    if case.kind in ("colmajor", "half"):  # k_sddmm_panels_f32: nothing is built
        assert not any(st["rb_items"]) and st["dense_sampled_tiles"] == 0 and st["ptile_items"] == 0


@pytest.mark.parametrize("name", ["half_K96_f16", "ptile_K64_f16"])
def test_half_panels_without_a_row_block_slot_are_unsupported(name):
    """fp16 / bf16 panel ranges exist only on the row-block launch: P stays untouched."""
    torch = torch_cuda()
    case = BY_NAME[name]
    K, dtype, nnz = case.K, case.dtype, len(pattern(case.pattern)[3])
    plan = _plan(case)
    A, B, _, _ = reference(case.pattern, K, dtype, "grid")
    dA, dB, dP = to_device(A, dtype), to_device(B, dtype), nan_output(nnz)
    for fn in (plan.sddmm_panels, plan.sddmm_panels_local):
        with pytest.raises(bsmr.BsmrError) as ei:
            fn(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), 0, 1, dtype=dtype)
        assert ei.value.status == UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(dP).all()


@pytest.mark.parametrize("name", ["rb_K128_f32", "rb_K256_bf16"])
def test_panels_local(name):
    """bsmr_sddmm_panels_local: each shard gets only its own A rows, in reordered order."""
    torch = torch_cuda()
    case = BY_NAME[name]
    pat = pattern(case.pattern)
    K, dtype, nnz = case.K, case.dtype, len(pat[3])
    plan = _plan(case)
    rows = plan.array("reorderedRows")
    s = torch.cuda.current_stream().cuda_stream
    ranges = _uneven_ranges(plan.stats()["num_row_panels"])
    for data in ("grid", "signed"):
        A, B, ref, S = reference(case.pattern, K, dtype, data)
        dB, dP = to_device(B, dtype), nan_output(nnz)
        done = np.zeros(nnz, bool)
        for p0, p1 in ranges:
            dA = to_device(A[rows[16 * p0:16 * p1]], dtype)
            plan.sddmm_panels_local(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), p0, p1, stream=s,
                                    dtype=dtype)
            torch.cuda.synchronize()
            done |= _written_by(plan, pat, p0, p1)
            assert np.array_equal(np.isfinite(dP.cpu().numpy()[:nnz]), done)
        P = dP.cpu().numpy()[:nnz]
        if data == "grid":
            assert_exact(P, ref, name + " local grid")
        else:
            assert_bound(P, ref, S, K, name + " local", case.kind + "/panels_local")


@pytest.mark.parametrize("name", ["rb_K128_f32", "dense_K64_bf16"])
def test_captured_first_launch_replayed_on_new_operands(name):
    """After Plan.prepare the plan's first launch is captured into a graph; the replay on grid data is
    exact, and a second replay after A and B were overwritten in place with signed data meets the
    bound (the graph reads the caller's buffers)."""
    torch = torch_cuda()
    case = BY_NAME[name]
    K, dtype, nnz = case.K, case.dtype, len(pattern(case.pattern)[3])
    plan = _plan(case)
    plan.prepare(K, dtype)
    assert plan.prepared(K, dtype)
    assert not path_evidence(case, plan)
    A, B, ref, _ = reference(case.pattern, K, dtype, "grid")
    dA, dB, dP = to_device(A, dtype), to_device(B, dtype), nan_output(nnz)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # a plain chain of nodes on a side stream
        plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), stream=side.cuda_stream, dtype=dtype)
    g.replay()
    torch.cuda.synchronize()
    assert_exact(dP.cpu().numpy()[:nnz], ref, name + " captured grid")
    A, B, ref, S = reference(case.pattern, K, dtype, "signed")
    dA.copy_(to_device(A, dtype))
    dB.copy_(to_device(B, dtype))
    dP.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert_bound(dP.cpu().numpy()[:nnz], ref, S, K, name + " replayed", case.kind + "/graph")
