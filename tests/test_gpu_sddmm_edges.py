"""GPU: the edges of the forward SDDMM (reference, data and bound: tests/sddmm_cases.py).

* the smallest legal plans (bsmr_plan_create needs nnz >= 2): M or N of 1 or 2, M around one
  16-row panel, a single full row, a 17 x 17 full mask; all three dtypes and layouts, grid data,
  bit equality;
* K / dtype combinations no launch supports, on every entry point: BSMR_ERR_UNSUPPORTED and P
  untouched;
* guard zones: A, B and P inside larger device buffers (4096 elements before and after; NaN around A
  and B, a fixed bit pattern around P): P exact, its guards unchanged. The guards are passive:
  nothing here reads or writes out of bounds on purpose;
* NaN in the A rows and B rows no stored entry references: P finite and within the bound;
* one referenced A row NaN and one referenced B row +inf: exactly that row's entries are NaN, that
  column's are non-finite, every other entry is finite and within the bound;
* scaled operands: fp16 data times 2^-12 and 2^-14 per operand (a quarter, then all, of the values
  are fp16 subnormals) and fp32 data times 2^-60: a subnormal input contributes its value on every
  path, and the bound's absolute term scales with the operands.
"""
import numpy as np
import pytest

import bsmr
from bsmr import BF16, F16, F32, Plan
from gpu_util import nan_output, path_evidence, sddmm_once, to_device, torch_cuda, torch_dtype
from sddmm_cases import (BY_NAME, DTYPE_NAME, FREE, ONE_PER_KIND, Case, as_seen, assert_bound, assert_exact,
                         grid_data, pattern, plan_kwargs, reference, sddmm_ref, signed_data)
from small_patterns import SMALL
from spmm_cases import entry_rows

pytestmark = pytest.mark.gpu

UNSUPPORTED = 6  # BSMR_ERR_UNSUPPORTED
GUARD = 4096
P_GUARD_BITS = 0x5A5AC3C3


@pytest.mark.parametrize("layout", ["auto", "rowblock", "colmajor"])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_smallest_plans(name, layout):
    pat = SMALL[name]
    M, N, rp, ci = pat
    nnz = len(ci)
    assert nnz >= 2
    plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, layout=layout)
    assert plan.stats()["nnz"] == nnz
    for K, dtype in ((16, F32), (32, F16), (64, F16), (32, BF16), (64, BF16)):
        A = grid_data(M * K, 5 + K).reshape(M, K)
        B = grid_data(N * K, 6 + K).reshape(N, K)
        ref, _ = sddmm_ref(pat, A, B)
        assert_exact(sddmm_once(plan, A, B, K, nnz, dtype), ref, f"{name} {layout} K={K} dtype={dtype}")


BAD_KD = [(24, F32, "auto"), (0, F32, "auto"), (32, 3, "auto"), (16, F16, "colmajor"),
          (48, BF16, "colmajor"), (80, F16, "colmajor")]


@pytest.mark.parametrize("K,dtype,layout", BAD_KD)
def test_unsupported_k_and_dtype_leave_p_untouched(K, dtype, layout):
    torch = torch_cuda()
    M, N, rp, ci = pattern("empty")
    plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, layout=layout)
    d = torch.zeros(3 * max(M, N) * 128, dtype=torch.float32, device="cuda")
    dP = nan_output(3 * len(ci))
    a, b, p = d.data_ptr(), d.data_ptr(), dP.data_ptr()
    npanels = plan.stats()["num_row_panels"]
    calls = {
        "sddmm": lambda: plan.sddmm(a, b, K, p, dtype=dtype),
        "sddmm_batch": lambda: plan.sddmm_batch(3, a, b, K, p, dtype=dtype),
        "sddmm_panels": lambda: plan.sddmm_panels(a, b, K, p, 0, npanels, dtype=dtype),
        "sddmm_panels_local": lambda: plan.sddmm_panels_local(a, b, K, p, 0, npanels, dtype=dtype),
        "prepare": lambda: plan.prepare(K, dtype),
        "prepare_panels": lambda: plan.prepare(K, dtype, panels=(0, npanels)),
    }
    for what, call in calls.items():
        with pytest.raises(bsmr.BsmrError) as ei:
            call()
        assert ei.value.status == UNSUPPORTED, (what, str(ei.value))
    assert not plan.prepared(K, dtype)
    torch.cuda.synchronize()
    assert torch.isnan(dP).all(), "a refused launch wrote P"
    st = plan.stats()
    assert not any(st["rb_items"]) and st["dense_sampled_tiles"] == 0 and st["ptile_items"] == 0


def _guarded(X, dtype):
    """X inside a NaN buffer with GUARD elements before and after: (buffer, view of the middle)."""
    torch = torch_cuda()
    X = to_device(X, dtype).reshape(-1)
    buf = torch.full((X.numel() + 2 * GUARD,), float("nan"), dtype=torch_dtype(dtype), device="cuda")
    mid = buf[GUARD:GUARD + X.numel()]
    mid.copy_(X)
    return buf, mid


@pytest.mark.parametrize("name", ONE_PER_KIND)
def test_guard_zones(name):
    torch = torch_cuda()
    case = BY_NAME[name]
    M, N, rp, ci = pattern(case.pattern)
    K, dtype, nnz = case.K, case.dtype, len(ci)
    plan = Plan(M, N, rp, ci, **plan_kwargs(case))
    A, B, ref, _ = reference(case.pattern, K, dtype, "grid")
    bufA, dA = _guarded(A, dtype)
    bufB, dB = _guarded(B, dtype)
    bufP = torch.full((nnz + 2 * GUARD,), P_GUARD_BITS, dtype=torch.int32, device="cuda")
    dP = bufP[GUARD:GUARD + nnz].view(torch.float32)
    dP.fill_(float("nan"))
    assert dA.data_ptr() % 16 == 0 and dB.data_ptr() % 16 == 0 and dP.data_ptr() % 16 == 0
    plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
               stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    host = bufP.cpu().numpy()
    assert (host[:GUARD] == P_GUARD_BITS).all(), "a store before P[0]"
    assert (host[GUARD + nnz:] == P_GUARD_BITS).all(), "a store past P[nnz)"
    assert_exact(host[GUARD:GUARD + nnz].view(np.float32), ref, name + " guarded")
    # the operands and their guards are read-only
    assert torch.isnan(bufA[:GUARD]).all() and torch.isnan(bufA[GUARD + dA.numel():]).all()
    assert torch.equal(dA, to_device(A, dtype).reshape(-1))
    assert torch.equal(dB, to_device(B, dtype).reshape(-1))
    assert not path_evidence(case, plan)


def _case(kind, pat, K, dtype, layout="auto", tuning=None):
    name = "_".join([kind, pat, f"K{K}", DTYPE_NAME[dtype]] + sorted(tuning or {}))
    return Case(name, kind, pat, K, dtype, layout, dict(tuning or {}), {}, None)


# launches over patterns with rows and columns nobody references: `empty` (69 empty rows, 260
# empty columns; dense-sampled by dense_min = 0) and `zipf` (619 empty columns; tiles whose last
# column group is padded with the sentinel column)
UNREFERENCED = [
    _case("colmajor", "empty", 48, F32), _case("colmajor", "zipf", 48, F32),
    _case("half", "empty", 96, F16), _case("half", "zipf", 96, BF16),
    _case("rowblock", "empty", 64, F32), _case("rowblock", "empty", 128, BF16),
    _case("rowblock", "zipf", 128, F32, tuning={"tile_min_f32": 0}),
    _case("rowblock", "empty", 128, F32, tuning={"col_blocks": 1}),
    _case("rowblock", "empty", 128, F32, tuning={"orig_rows": 1}),
    _case("dense", "empty", 64, F16, tuning={"dense_min": 0.0}),
    _case("ptile", "zipf", 128, F16, tuning={"ptile": 1}),
]


def _built_kind(st):
    return ("rowblock" if any(st["rb_items"]) else "dense" if st["dense_sampled_tiles"] else
            "ptile" if st["ptile_items"] else "colmajor")


@pytest.mark.parametrize("case", UNREFERENCED, ids=[c.name for c in UNREFERENCED])
def test_unreferenced_rows_may_hold_nan(case):
    pat = pattern(case.pattern)
    M, N, rp, ci = pat
    K, dtype, nnz = case.K, case.dtype, len(ci)
    A = signed_data(M * K, 31).reshape(M, K)
    B = signed_data(N * K, 32).reshape(N, K)
    A[np.diff(rp.astype(np.int64)) == 0] = np.nan
    B[np.bincount(ci, minlength=N) == 0] = np.nan
    assert np.isnan(B).any() and (case.pattern != "empty" or np.isnan(A).any())
    A, B = as_seen(A, dtype), as_seen(B, dtype)
    ref, S = sddmm_ref(pat, A, B)
    assert np.isfinite(ref).all()
    plan = Plan(M, N, rp, ci, **plan_kwargs(case))
    P = sddmm_once(plan, A, B, K, nnz, dtype)
    assert_bound(P, ref, S, K, case.name + " unreferenced NaN", case.kind + "/nan_unreferenced")
    assert _built_kind(plan.stats()) == {"half": "colmajor"}.get(case.kind, case.kind)


NON_FINITE = ONE_PER_KIND + ["rb_tiles_K128_f32", "rb_col_blocks_K128_f32", "rb_pairs_K256_bf16",
                             "rbx_full_dyn_nt512_K64_f16", "cm_blocky_K128_f32"]


@pytest.mark.parametrize("name", NON_FINITE)
def test_non_finite_operands_stay_in_their_row_and_column(name):
    case = BY_NAME[name]
    pat = pattern(case.pattern)
    M, N, rp, ci = pat
    K, dtype, nnz = case.K, case.dtype, len(ci)
    A, B, _, _ = reference(case.pattern, K, dtype, "signed")
    A, B = A.copy(), B.copy()
    lens = np.diff(rp.astype(np.int64))
    r = int(np.nonzero(lens[M // 2:] >= 2)[0][0] + M // 2)  # a referenced row of the last panels
    c = int(np.bincount(ci, minlength=N).argmax())  # the most referenced column (in dense tiles)
    A[r] = np.nan
    B[c] = np.inf
    ref, S = sddmm_ref(pat, A, B)
    in_row = entry_rows(M, rp) == r
    in_col = np.asarray(ci) == c
    assert in_row.sum() >= 2 and in_col.sum() >= 2 and (~(in_row | in_col)).sum() > nnz // 2
    plan = Plan(M, N, rp, ci, **plan_kwargs(case))
    P = sddmm_once(plan, A, B, K, nnz, dtype)
    assert np.isnan(P[in_row]).all(), f"{name}: an entry of the NaN row is not NaN"
    assert not np.isfinite(P[in_col]).any(), f"{name}: an entry of the inf column is finite"
    rest = ~(in_row | in_col)
    bad = np.nonzero(rest & ~np.isfinite(P))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} entries beside the row and the column are not finite: {bad[:8]}"
    assert_bound(P[rest], ref[rest], S[rest], K, name + " beside NaN / inf", case.kind + "/non_finite")
    assert not path_evidence(case, plan)


# (case, log2 of the per-operand scaling): fp16 on every launch that takes it (MFMA tiles, the
# v_dot2 residual of the row-block kernel with and without kept tiles, dense-sampled, panel-tile),
# fp32 on the FMA and the fp32-MFMA paths
SCALED_F16 = ["half_K96_f16", "half_blocky_K128_f16", "rb_K256_f16", "rb_K64_f16", "rb_K1024_f16",
              "rbx_pair_nt1024_K1024_f16", "rb_col_blocks_K256_bf16", "dense_K64_f16", "ptile_K64_f16",
              "ptile_residual_K128_f16"]
SCALED_F32 = ["cm_K48_f32", "cm_K128_f32", "cm_blocky_K128_f32", "rb_K128_f32", "rb_K512_f32", "rb_tiles_K128_f32"]
SCALED = [(n, e) for n in SCALED_F16 for e in (-12, -14)] + [(n, -60) for n in SCALED_F32]


@pytest.mark.parametrize("name,exp", SCALED, ids=[f"{n}_2^{e}" for n, e in SCALED])
def test_scaled_operands(name, exp):
    case = BY_NAME[name]
    pat = pattern(case.pattern)
    M, N, rp, ci = pat
    K, dtype, nnz = case.K, case.dtype, len(ci)
    if exp > -60:
        dtype = F16  # the fp16 subnormal range (bf16 shares fp32's exponent)
    f = np.float32(2.0 ** exp)
    A = as_seen(signed_data(M * K, 41).reshape(M, K) * f, dtype)
    B = as_seen(signed_data(N * K, 42).reshape(N, K) * f, dtype)
    if dtype == F16:
        sub = float((np.abs(A) < 2.0 ** -14).mean())
        assert sub > (0.2 if exp == -12 else 0.999), sub  # fp16 subnormals (and zeros)
        assert (A != 0).mean() > 0.99
    ref, S = sddmm_ref(pat, A, B)
    plan = Plan(M, N, rp, ci, **plan_kwargs(case))
    P = sddmm_once(plan, A, B, K, nnz, dtype)
    assert_bound(P, ref, S, K, f"{name} x 2^{exp}", case.kind + "/scaled", scale=float(f) ** 2)
    assert not path_evidence(case._replace(dtype=dtype), plan)
