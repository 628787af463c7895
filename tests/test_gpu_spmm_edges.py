"""GPU: the edges of the plan-based SpMM (reference, data and bound: tests/spmm_cases.py). Grid
data and bit equality wherever the data allow it.

* the smallest legal plans (tests/small_patterns.py), both sides, K = 16 fp32, K = 16 and 64 fp16,
  K = 32 bf16: bit-exact;
* guard zones: V, X and Y inside larger device buffers (4096 elements before and after; NaN
  around V and X, a fixed bit pattern around Y), every pointer 16-byte aligned, a fixed and a
  generic case on `hub` at chunk 32 (the partial-row path): Y exact, its guards bit-identical, V
  and X and their guards unchanged. The guards are passive: nothing here reads or writes out of
  bounds on purpose;
* NaN in the source rows no stored entry references (side 1: the B rows of columns without
  entries, side 2: the A rows of empty rows): Y finite and within the tight bound;
* non-finite containment, on `hub` at chunk 32 (through the partial rows and k_spmm_reduce) and on
  `zipf` at the default chunk: one V entry of the longest row NaN: exactly that row (side 1) or that
  entry's column (side 2) is NaN in every column of Y; one referenced X row +inf: exactly the
  destinations whose list holds that source are non-finite in every column; everything else
  finite and within the tight bound;
* scaled operands: fp16 X times 2^-12 and 2^-14 (subnormals) with a standard normal V, fp32 V
  and X each times 2^-60; the bound's absolute term scales with the product of the scalings;
* one plan prepared at K = 32, chunk 32, then launched at (512, fp32), (64, bf16), (1024, fp16),
  (32, fp32): the first launch grows the scratch; every result bitwise equal to a fresh plan's;
* the two sides on two streams (inputs made ready with an event, no graph capture): bitwise equal
  to the serial results.
"""
import numpy as np
import pytest

from bsmr import BF16, F16, F32, Plan
from gpu_util import spmm_device, spmm_launch, spmm_once, to_device, torch_cuda, torch_dtype
from sddmm_cases import as_seen, grid_data, signed_data
from small_patterns import SMALL
from spmm_cases import (assert_exact, assert_tight, case_id, entry_rows, expected_stats, grid_values, list_lengths,
                        pattern, signed_values, spmm_form, spmm_ref)

pytestmark = pytest.mark.gpu

FREE = 288 * 1024 ** 3
GUARD = 4096
Y_GUARD_BITS = 0x5A5AC3C3
FIXED_AND_GENERIC = [(128, F32), (48, BF16)]  # k_spmm<f32, 32, 1> and the generic form at L = 8, 6 live
KD_IDS = [case_id(*kd) for kd in FIXED_AND_GENERIC]


def _plan(pat):
    M, N, rp, ci = pat
    return Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE)


def _source_rows(pat, side):
    return pat[1] if side == 1 else pat[0]


def _signed(pat, side, K, dtype, seed=50):
    """(V, X as the kernel sees it) of one side, signed data."""
    rows = _source_rows(pat, side)
    return signed_values(len(pat[3]), seed), as_seen(signed_data(rows * K, seed + side).reshape(rows, K), dtype)


def test_the_two_cases_are_a_fixed_and_a_generic_form():
    assert [spmm_form(K, d)["fixed"] for K, d in FIXED_AND_GENERIC] == [True, False]


@pytest.mark.parametrize("name", sorted(SMALL))
def test_smallest_plans(name):
    pat = SMALL[name]
    nnz = len(pat[3])
    assert nnz >= 2
    plan = _plan(pat)
    for K, dtype in ((16, F32), (16, F16), (64, F16), (32, BF16)):
        for side in (1, 2):
            rows = _source_rows(pat, side)
            V, X = grid_values(nnz, 7 + K), grid_data(rows * K, 8 + K + side).reshape(rows, K)
            Y = spmm_once(plan, side, V, X, K, dtype)
            assert_exact(Y, spmm_ref(pat, side, V, X), f"{name} K={K} dtype={dtype} side {side}")
    for side in (1, 2):
        assert plan.spmm_stats(side) == expected_stats(pat, side, 128)


def _guarded(X, dtype, fill=float("nan")):
    """X inside a buffer of `fill` with GUARD elements before and after: (buffer, view of the middle)."""
    torch = torch_cuda()
    X = to_device(X, dtype).reshape(-1)
    buf = torch.full((X.numel() + 2 * GUARD,), fill, dtype=torch_dtype(dtype), device="cuda")
    mid = buf[GUARD:GUARD + X.numel()]
    mid.copy_(X)
    return buf, mid


def _bits(t):
    torch = torch_cuda()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("K,dtype", FIXED_AND_GENERIC, ids=KD_IDS)
def test_guard_zones(K, dtype):
    torch = torch_cuda()
    pat = pattern("hub")
    M, N, _, ci = pat
    plan = _plan(pat)
    plan.prepare_spmm(K, 3, chunk=32)
    V = grid_values(len(ci), 61)
    for side in (1, 2):
        assert plan.spmm_stats(side) == expected_stats(pat, side, 32)
        rows, dsts = _source_rows(pat, side), (M if side == 1 else N)
        X = grid_data(rows * K, 62 + side).reshape(rows, K)
        ref = spmm_ref(pat, side, V, X)
        bufV, dV = _guarded(V, F32)
        bufX, dX = _guarded(X, dtype)
        bufY = torch.full((dsts * K + 2 * GUARD,), Y_GUARD_BITS, dtype=torch.int32, device="cuda")
        dY = bufY[GUARD:GUARD + dsts * K].view(torch.float32)
        dY.fill_(float("nan"))
        assert dV.data_ptr() % 16 == 0 and dX.data_ptr() % 16 == 0 and dY.data_ptr() % 16 == 0
        keepV, keepX = _bits(bufV).clone(), _bits(bufX).clone()
        spmm_launch(plan, side, dV, dX, K, dtype, dY)
        torch.cuda.synchronize()
        host = bufY.cpu().numpy()
        assert (host[:GUARD] == Y_GUARD_BITS).all(), f"side {side}: a store before Y[0]"
        assert (host[GUARD + dsts * K:] == Y_GUARD_BITS).all(), f"side {side}: a store past Y"
        assert_exact(host[GUARD:GUARD + dsts * K].view(np.float32).reshape(dsts, K), ref, f"guarded side {side}")
        # the operands and their guards are read-only
        assert torch.equal(_bits(bufV), keepV) and torch.equal(_bits(bufX), keepX)
        assert torch.isnan(bufV[:GUARD]).all() and torch.isnan(bufX[GUARD + dX.numel():]).all()


@pytest.mark.parametrize("K,dtype", FIXED_AND_GENERIC, ids=KD_IDS)
@pytest.mark.parametrize("name,side", [("empty", 1), ("empty", 2), ("zipf", 1)])
def test_unreferenced_source_rows_may_hold_nan(name, side, K, dtype):
    pat = pattern(name)
    V, X = _signed(pat, side, K, dtype)
    X = X.copy()
    unreferenced = list_lengths(pat, 3 - side) == 0  # side 1: columns without entries; side 2: empty rows
    assert unreferenced.sum() >= 60
    X[unreferenced] = np.nan
    ref = spmm_ref(pat, side, V, X)
    assert np.isfinite(ref[0]).all()
    Y = spmm_once(_plan(pat), side, V, X, K, dtype)
    assert_tight(Y, ref, f"{name} {case_id(K, dtype)} side {side}", "nan_unreferenced")


def _check_contained(Y, ref, affected, what, kind):
    """Exactly the `affected` destinations are non-finite, in every column; the rest is finite and
    within the tight bound. The reference must agree on the affected set first."""
    Yr, S, n = ref
    assert np.array_equal(~np.isfinite(Yr).all(axis=1), affected) and not np.isfinite(Yr[affected]).any()
    assert 0 < affected.sum() < len(affected) / 2
    assert not np.isfinite(Y[affected]).any(), f"{what}: an affected element is finite"
    rest = ~affected
    bad = np.nonzero(~np.isfinite(Y[rest]).all(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} destinations beside the affected ones are not finite"
    assert_tight(Y[rest], (Yr[rest], S[rest], n[rest]), what, kind)


@pytest.mark.parametrize("K,dtype", FIXED_AND_GENERIC, ids=KD_IDS)
@pytest.mark.parametrize("name,chunk", [("hub", 32), ("zipf", 0)])
def test_non_finite_values_stay_in_their_destinations(name, chunk, K, dtype):
    pat = pattern(name)
    M, N, rp, ci = pat
    plan = _plan(pat)
    plan.prepare_spmm(K, 3, chunk=chunk)
    rows_of, cols_of = entry_rows(M, rp), np.asarray(ci, np.int64)
    hub = int(list_lengths(pat, 1).argmax())
    e = int(rp[hub]) + int(rp[hub + 1] - rp[hub]) // 2  # an entry in the middle of the longest row
    with np.errstate(invalid="ignore", over="ignore"):
        for side in (1, 2):
            D = M if side == 1 else N
            dst, src = (rows_of, cols_of) if side == 1 else (cols_of, rows_of)
            what = f"{name} {case_id(K, dtype)} chunk {chunk} side {side}"
            # one NaN value
            V, X = _signed(pat, side, K, dtype)
            V[e] = np.nan
            affected = np.zeros(D, bool)
            affected[dst[e]] = True
            Y = spmm_once(plan, side, V, X, K, dtype)
            _check_contained(Y, spmm_ref(pat, side, V, X), affected, what + " NaN in V", "non_finite")
            assert np.isnan(Y[affected]).all(), f"{what}: the NaN value's destination is not NaN"
            # one +inf source row: the most referenced source that under half of the destinations hold
            V, X = _signed(pat, side, K, dtype)
            X = X.copy()
            refs = np.bincount(src, minlength=_source_rows(pat, side))
            s = int(np.where(refs < D // 4, refs, 0).argmax())
            assert refs[s] >= 2
            X[s] = np.inf
            affected = np.zeros(D, bool)
            affected[dst[src == s]] = True
            Y = spmm_once(plan, side, V, X, K, dtype)
            _check_contained(Y, spmm_ref(pat, side, V, X), affected, what + " inf row of X", "non_finite")


SCALED = [(128, F16, -12), (128, F16, -14), (48, F16, -12), (48, F16, -14), (128, F32, -60), (48, F32, -60)]


@pytest.mark.parametrize("K,dtype,exp", SCALED, ids=[f"{case_id(K, d)}_2^{e}" for K, d, e in SCALED])
def test_scaled_operands(K, dtype, exp):
    pat = pattern("zipf")
    nnz = len(pat[3])
    plan = _plan(pat)
    f = np.float32(2.0 ** exp)
    V = np.random.default_rng(71).standard_normal(nnz).astype(np.float32)
    if dtype == F32:
        V *= f
    for side in (1, 2):
        rows = _source_rows(pat, side)
        X = as_seen(signed_data(rows * K, 72 + side).reshape(rows, K) * f, dtype)
        if dtype == F16:
            sub = float((np.abs(X) < 2.0 ** -14).mean())
            assert sub > (0.2 if exp == -12 else 0.999), sub  # fp16 subnormals (and zeros)
            assert (X != 0).mean() > 0.99
        scale = float(f) ** (2 if dtype == F32 else 1)
        Y = spmm_once(plan, side, V, X, K, dtype)
        assert (Y != 0).mean() > 0.5  # (a seventh of the columns is empty)
        assert_tight(Y, spmm_ref(pat, side, V, X), f"zipf {case_id(K, dtype)} x 2^{exp} side {side}", "scaled",
                     scale=scale)


def test_one_plan_reused_across_k_and_dtype():
    torch_cuda()
    pat = pattern("hub")
    nnz = len(pat[3])
    plan = _plan(pat)
    plan.prepare_spmm(32, 3, chunk=32)
    assert plan.spmm_prepared(32, 3) and plan.spmm_prepared(16, 3)
    assert not plan.spmm_prepared(512, 1)  # the hub row's partial rows need a larger scratch
    V = signed_values(nnz, 81)
    done = []
    for K, dtype in ((512, F32), (64, BF16), (1024, F16), (32, F32)):
        fresh = _plan(pat)
        fresh.prepare_spmm(K, 3, chunk=32)
        for side in (1, 2):
            rows = _source_rows(pat, side)
            X = as_seen(signed_data(rows * K, 82 + side).reshape(rows, K), dtype)
            Y = spmm_once(plan, side, V, X, K, dtype)
            assert np.isfinite(Y).all()
            assert np.array_equal(Y, spmm_once(fresh, side, V, X, K, dtype)), (K, dtype, side)
            assert plan.spmm_stats(side) == expected_stats(pat, side, 32)  # the lists were kept
        done.append(K)
        assert all(plan.spmm_prepared(k, 3) for k in done) and plan.spmm_prepared(max(done) // 2, 3)
    assert not plan.spmm_prepared(2048, 1)


@pytest.mark.parametrize("name,chunk", [("hub", 32), ("zipf", 0)])
def test_the_two_sides_on_two_streams(name, chunk):
    torch = torch_cuda()
    pat = pattern(name)
    M, N, _, ci = pat
    K, dtype = 128, F32
    plan = _plan(pat)
    plan.prepare_spmm(K, 3, chunk=chunk)
    V = grid_values(len(ci), 91)
    A, B = grid_data(M * K, 92).reshape(M, K), grid_data(N * K, 93).reshape(N, K)
    dV, dA, dB = to_device(V, F32), to_device(A, dtype), to_device(B, dtype)
    serial = spmm_device(plan, 1, dV, dB, K, dtype), spmm_device(plan, 2, dV, dA, K, dtype)
    assert_exact(serial[0], spmm_ref(pat, 1, V, B), name + " serial side 1")
    assert_exact(serial[1], spmm_ref(pat, 2, V, A), name + " serial side 2")
    dY1 = torch.full((M, K), float("nan"), dtype=torch.float32, device="cuda")
    dY2 = torch.full((N, K), float("nan"), dtype=torch.float32, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ready = torch.cuda.Event()
    ready.record()  # the operands and the NaN fill, on the current stream
    s1.wait_event(ready)
    s2.wait_event(ready)
    spmm_launch(plan, 1, dV, dB, K, dtype, dY1, stream=s1)
    spmm_launch(plan, 2, dV, dA, K, dtype, dY2, stream=s2)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(dY1.cpu().numpy(), serial[0]) and np.array_equal(dY2.cpu().numpy(), serial[1])
