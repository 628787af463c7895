"""GPU: the plan-based SpMM (bsmr_spmm / bsmr_spmm_t; Plan.spmm / Plan.spmm_t), i.e. the gradients
dA = S(G) B and dB = S(G)^T A of the SDDMM.

Patterns (tests/spmm_cases.py): Zipf columns (M not a multiple of 16, longest column list 517,
619 empty columns), empty rows and columns, one hub row holding every column, and the Zipf
pattern with the columns of each row in file order. (K, dtype) cases cover the generic strided
kernel (rows of 64, 160, 192 bytes, and 1280 bytes = two column tiles), the five fixed row sizes
(128 B .. 2 KiB) and the two-chunk 2 KiB row.

Reference: float64 numpy from the CSR on the operands as the kernel sees them (fp16 / bf16
rounded by gpu_util.half_values).
  * positive data (make_data operands and values): the project's checkData rule, 0 mismatches;
  * signed data (V standard normal, operands make_data - 1): per element
    |Y - ref| <= 2 n 2^-24 sum|v x| + 1e-6, n the destination's list length: the standard bound of
    an n-term fp32 sum of once-rounded products (the kernel's FMAs round once per term), derived
    and not tuned;
  * Y starts as NaN and ends finite everywhere, exactly 0 for empty rows / columns;
  * default chunk and chunk 32 (split destinations through partial rows), with the stats;
  * two launches, and a lazily built against a prepared plan, are bitwise equal;
  * first launches capture after prepare_spmm, and report NOT_PREPARED without it;
  * recolumn keeps the lists; K / dtype / sides validation.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
import bsmr
from bsmr import BF16, F16, F32, Plan, make_data
from gpu_util import half_values, torch_cuda
from spmm_cases import PATTERNS, pattern, signed_bound, spmm_ref

pytestmark = pytest.mark.gpu

FREE = 288 * 1024 ** 3
# the issue's eight cases, then the two fixed sizes they leave out (128 B, 1 KiB rows) and a
# generic row over 1 KiB (two column tiles)
KD = [(16, F32), (48, F32), (128, F32), (512, F32), (32, F16), (80, BF16), (128, BF16), (1024, F16),
      (32, F32), (256, F32), (320, F32)]
DEFAULT_CHUNK = 128  # csrc/spmm_schedule.hpp SPMM_CHUNK_DEFAULT (what chunk = 0 builds on a fresh plan)


def _tdt(torch, dtype):
    return {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}[dtype]


def _dev(torch, X, dtype):
    return torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda().to(_tdt(torch, dtype))


def _nan(torch, rows, K):
    return torch.full((rows, K), float("nan"), dtype=torch.float32, device="cuda")


def _plan(name):
    M, N, rp, ci = pattern(name)
    return Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE)


@functools.lru_cache(maxsize=4)
def _data(name, K, dtype, signed):
    """Host operands as the kernel sees them and the float64 references of both sides; built
    once and shared (read-only) by the chunk variants."""
    pat = pattern(name)
    M, N, _, ci = pat
    nnz = len(ci)
    shift = np.float32(1.0) if signed else np.float32(0.0)
    A = (make_data(M * K) - shift).reshape(M, K)
    B = (make_data(N * K)[::-1].copy() - shift).reshape(N, K)
    if dtype != F32:
        A, B = half_values(A, dtype), half_values(B, dtype)
    V = np.random.default_rng(17).standard_normal(nnz).astype(np.float32) if signed else make_data(nnz)
    return A, B, V, spmm_ref(pat, 1, V, B), spmm_ref(pat, 2, V, A)


def _run(torch, plan, side, dV, dX, K, dtype, rows):
    dY = _nan(torch, rows, K)
    fn = plan.spmm if side == 1 else plan.spmm_t
    fn(dV.data_ptr(), dX.data_ptr(), K, dY.data_ptr(), stream=torch.cuda.current_stream().cuda_stream,
       dtype=dtype)
    torch.cuda.synchronize()
    return dY.cpu().numpy()


def _check(Y, ref, signed, what):
    Yr, S, n = ref
    assert np.isfinite(Y).all(), f"{what}: {int((~np.isfinite(Y)).sum())} elements never written"
    assert (Y[n == 0] == 0).all(), f"{what}: an empty destination is not exactly 0"
    if signed:
        err = np.abs(Y.astype(np.float64) - Yr)
        bound = signed_bound(S, n)
        worst = float((err / bound).max())
        print(f"{what}: max |Y - ref| / bound = {worst:.3f}")
        assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements over the bound ({worst:.2f} x)"
    else:
        assert O.check_data(Yr.astype(np.float32), Y) == 0, what


@pytest.mark.parametrize("K,dtype", KD, ids=[f"K{k}_{'f32 f16 bf16'.split()[d]}" for k, d in KD])
@pytest.mark.parametrize("name", PATTERNS)
def test_spmm_matches_float64(name, K, dtype):
    torch = torch_cuda()
    M, N, _, _ = pattern(name)
    plan = _plan(name)
    for signed in (False, True):
        A, B, V, ref1, ref2 = _data(name, K, dtype, signed)
        dA, dB = _dev(torch, A, dtype), _dev(torch, B, dtype)
        dV = torch.from_numpy(V).cuda()
        for chunk in (DEFAULT_CHUNK, 32):
            plan.prepare_spmm(K, 3, chunk=chunk)
            assert plan.spmm_prepared(K, 3)
            assert plan.spmm_stats(1)["chunk"] == plan.spmm_stats(2)["chunk"] == chunk
            what = f"{name} K={K} dtype={dtype} signed={signed} chunk={chunk}"
            _check(_run(torch, plan, 1, dV, dB, K, dtype, M), ref1, signed, what + " side 1")
            _check(_run(torch, plan, 2, dV, dA, K, dtype, N), ref2, signed, what + " side 2")


def test_chunk_stats_show_the_split_paths():
    from spmm_cases import entry_rows
    for name, side, longest in (("zipf", 2, 517), ("hub", 1, 2048)):
        M, N, rp, ci = pattern(name)
        plan = _plan(name)
        assert plan.spmm_stats(side) == dict(segments=0, split_dsts=0, partials=0, max_list=0, chunk=0)
        plan.prepare_spmm(64, 3, chunk=32)
        st = plan.spmm_stats(side)
        lens = np.bincount(ci if side == 2 else entry_rows(M, rp), minlength=N if side == 2 else M)
        nseg = np.maximum(1, -(-lens // 32))
        assert st["chunk"] == 32 and st["max_list"] == longest == lens.max()
        assert st["split_dsts"] == int((nseg > 1).sum()) > 0
        assert st["partials"] == int(nseg[nseg > 1].sum())
        assert st["segments"] == int(nseg.sum())
        # chunk 0 keeps what is built; the default chunk rebuilds
        plan.prepare_spmm(64, 3)
        assert plan.spmm_stats(side)["chunk"] == 32
        plan.prepare_spmm(64, 3, chunk=DEFAULT_CHUNK)
        st = plan.spmm_stats(side)
        assert st["chunk"] == DEFAULT_CHUNK and st["split_dsts"] == int((lens > DEFAULT_CHUNK).sum())


@pytest.mark.parametrize("name,K,dtype,chunk", [("zipf", 128, F32, 32), ("hub", 128, BF16, 32),
                                                ("hub", 48, F32, DEFAULT_CHUNK)])
def test_bitwise_reproducible(name, K, dtype, chunk):
    torch = torch_cuda()
    M, N, _, _ = pattern(name)
    A, B, V, _, _ = _data(name, K, dtype, True)
    dA, dB, dV = _dev(torch, A, dtype), _dev(torch, B, dtype), torch.from_numpy(V).cuda()
    prepared = _plan(name)
    prepared.prepare_spmm(K, 3, chunk=chunk)
    outs = [(_run(torch, prepared, 1, dV, dB, K, dtype, M), _run(torch, prepared, 2, dV, dA, K, dtype, N))
            for _ in range(2)]
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    if chunk == DEFAULT_CHUNK:  # a lazy build uses the default chunk
        lazy = _plan(name)
        assert not lazy.spmm_prepared(K, 1) and not lazy.spmm_prepared(K, 2)
        y1 = _run(torch, lazy, 1, dV, dB, K, dtype, M)
        assert lazy.spmm_prepared(K, 1) and not lazy.spmm_prepared(K, 2)
        y2 = _run(torch, lazy, 2, dV, dA, K, dtype, N)
        assert lazy.spmm_prepared(K, 3)
        assert np.array_equal(y1, outs[0][0]) and np.array_equal(y2, outs[0][1])


def _capture(torch, fn):
    """fn(stream) recorded into a graph on a side stream (a plain chain of nodes)."""
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(side.cuda_stream)
    return g


@pytest.mark.parametrize("name,K,dtype,chunk", [("zipf", 128, F32, 32), ("hub", 128, F16, 0)])
def test_first_launches_captured_after_prepare(name, K, dtype, chunk):
    torch = torch_cuda()
    pat = pattern(name)
    M, N, _, _ = pat
    A, B, V, ref1, ref2 = _data(name, K, dtype, True)
    plan = _plan(name)
    assert not plan.spmm_prepared(K, 3)
    plan.prepare_spmm(K, 3, chunk=chunk)
    assert plan.spmm_prepared(K, 3) and plan.spmm_prepared(K // 2, 3)  # the scratch covers smaller K
    assert plan.spmm_stats(1)["chunk"] == (chunk or DEFAULT_CHUNK)
    dA, dB, dV = _dev(torch, A, dtype), _dev(torch, B, dtype), torch.from_numpy(V).cuda()
    dY1, dY2 = _nan(torch, M, K), _nan(torch, N, K)
    torch.cuda.synchronize()

    def body(s):
        plan.spmm(dV.data_ptr(), dB.data_ptr(), K, dY1.data_ptr(), stream=s, dtype=dtype)
        plan.spmm_t(dV.data_ptr(), dA.data_ptr(), K, dY2.data_ptr(), stream=s, dtype=dtype)

    g = _capture(torch, body)
    g.replay()
    torch.cuda.synchronize()
    _check(dY1.cpu().numpy(), ref1, True, "captured side 1")
    _check(dY2.cpu().numpy(), ref2, True, "captured side 2")
    # the graph reads the caller's V, not a captured copy
    V2 = (V[::-1] * np.float32(0.5)).copy()
    dV.copy_(torch.from_numpy(V2).cuda())
    dY1.fill_(float("nan"))
    dY2.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    _check(dY1.cpu().numpy(), spmm_ref(pat, 1, V2, B), True, "replayed side 1")
    _check(dY2.cpu().numpy(), spmm_ref(pat, 2, V2, A), True, "replayed side 2")


@pytest.mark.parametrize("side", [1, 2])
def test_unprepared_capture_reports_not_prepared(side):
    torch = torch_cuda()
    name, K, dtype = "empty", 64, F32
    M, N, _, _ = pattern(name)
    A, B, V, ref1, ref2 = _data(name, K, dtype, True)
    plan = _plan(name)
    dX = _dev(torch, B if side == 1 else A, dtype)
    dV = torch.from_numpy(V).cuda()
    dY = _nan(torch, M if side == 1 else N, K)
    fn = plan.spmm if side == 1 else plan.spmm_t
    torch.cuda.synchronize()
    caught = []

    def body(s):
        dY.zero_()
        with pytest.raises(bsmr.BsmrError) as ei:
            fn(dV.data_ptr(), dX.data_ptr(), K, dY.data_ptr(), stream=s, dtype=dtype)
        caught.append(ei.value)

    g = _capture(torch, body)  # ends normally: the refused launch did not invalidate the capture
    assert caught[0].status == bsmr.NOT_PREPARED
    assert ("bsmr_spmm: " if side == 1 else "bsmr_spmm_t: ") + "stream is capturing" in str(caught[0])
    assert "bsmr_plan_prepare_spmm first" in str(caught[0])
    g.replay()
    torch.cuda.synchronize()
    assert (dY.cpu().numpy() == 0).all()
    assert not plan.spmm_prepared(K, side)
    # outside capture the same call builds lazily
    Y = _run(torch, plan, side, dV, dX, K, dtype, M if side == 1 else N)
    _check(Y, ref1 if side == 1 else ref2, True, f"lazy side {side}")
    assert plan.spmm_prepared(K, side) and not plan.spmm_prepared(K, 3 - side)


def test_recolumn_keeps_the_lists():
    torch = torch_cuda()
    name, K, dtype = "zipf", 64, F32
    M, N, _, _ = pattern(name)
    A, B, V, _, _ = _data(name, K, dtype, True)
    dA, dB, dV = _dev(torch, A, dtype), _dev(torch, B, dtype), torch.from_numpy(V).cuda()
    plan = _plan(name)
    plan.prepare_spmm(K, 3, chunk=32)
    before = (_run(torch, plan, 1, dV, dB, K, dtype, M), _run(torch, plan, 2, dV, dA, K, dtype, N))
    stats = (plan.spmm_stats(1), plan.spmm_stats(2))
    plan.recolumn(0.5)
    assert plan.spmm_prepared(K, 3)
    assert (plan.spmm_stats(1), plan.spmm_stats(2)) == stats
    after = (_run(torch, plan, 1, dV, dB, K, dtype, M), _run(torch, plan, 2, dV, dA, K, dtype, N))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_validation():
    torch = torch_cuda()
    M, N, _, ci = pattern("empty")
    plan = _plan("empty")
    UNSUPPORTED, INVALID = 6, 1
    d = torch.zeros(max(M, N) * 32, dtype=torch.float32, device="cuda")
    v = torch.zeros(len(ci), dtype=torch.float32, device="cuda")
    for fn in (plan.spmm, plan.spmm_t):
        for K, dtype in ((24, F32), (0, F32), (32, 3), (32, -1)):
            with pytest.raises(bsmr.BsmrError) as ei:
                fn(v.data_ptr(), d.data_ptr(), K, d.data_ptr(), dtype=dtype)
            assert ei.value.status == UNSUPPORTED, str(ei.value)
        with pytest.raises(bsmr.BsmrError) as ei:
            fn(0, d.data_ptr(), 32, d.data_ptr())
        assert ei.value.status == INVALID
    with pytest.raises(bsmr.BsmrError) as ei:
        plan.prepare_spmm(24, 3)
    assert ei.value.status == UNSUPPORTED
    for sides in (0, 4, -1):
        with pytest.raises(bsmr.BsmrError) as ei:
            plan.prepare_spmm(32, sides)
        assert ei.value.status == INVALID and "bsmr_plan_prepare_spmm" in str(ei.value)
        assert not plan.spmm_prepared(32, sides)
    with pytest.raises(bsmr.BsmrError) as ei:
        plan.spmm_stats(3)
    assert ei.value.status == INVALID
    assert not plan.spmm_prepared(32, 3)
