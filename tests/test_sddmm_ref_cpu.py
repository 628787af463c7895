"""CPU: the checker of the forward SDDMM tests checks itself (tests/sddmm_cases.py).

* sddmm_ref (float64 numpy) against bsmr.sddmm_cpu (the host fp32 loop, include/bsmr.h
  bsmr_sddmm_cpu): within sddmm_bound on signed data, bit-equal on grid data.
* Four kernel mutations applied to the host result: the result rounded to fp16 once, fp32 inputs cut
  to 10 mantissa bits, the last k element dropped, the last 4 k elements taken from the
  neighbouring B row. Each fails the bound on signed data at every K; those that change a value
  fail bit equality on grid data. This pins the tolerance: a bound loose enough to pass one of them
  fails here.
* grid_data survives the fp16 / bf16 rounding unchanged; the bound's two regimes; the case table
  names every launch kind and every row size; bsmr_plan_create refuses nnz < 2 before any device
  call.
"""
import numpy as np
import pytest

import bsmr
from bsmr import BF16, F16, F32
from gpu_util import half_values
from sddmm_cases import (BY_NAME, CASES, ONE_PER_KIND, PANEL_CASES, bound_ratio, grid_data, pattern,
                         rb_slot, sddmm_bound, sddmm_ref, signed_data)

KS = [16, 128, 512, 1024]


def _host(pat, A, B):
    M, N, rp, ci = pat
    return bsmr.sddmm_cpu(M, N, rp, ci, A.shape[1], A, B, threads=4)


def _operands(pat, K, gen):
    M, N, _, _ = pat
    return gen(M * K, 11).reshape(M, K), gen(N * K, 12).reshape(N, K)


def _cut_mantissa(X, bits=10):
    drop = np.uint32(23 - bits)
    return ((X.view(np.uint32) >> drop) << drop).view(np.float32)


def _mutations(pat, A, B):
    """name -> (mutated host result, whether the mutation changes a value on 6-bit grid data)."""
    N = pat[1]
    P = _host(pat, A, B)
    A_drop = A.copy()
    A_drop[:, -1] = 0
    B_shift = B.copy()
    B_shift[:, -4:] = B[(np.arange(N) + 1) % N, -4:]
    return {
        "result rounded to fp16": (P.astype(np.float16).astype(np.float32), True),
        "inputs cut to 10 mantissa bits": (_host(pat, _cut_mantissa(A), _cut_mantissa(B)), False),
        "last k dropped": (_host(pat, A_drop, B), True),
        "last 4 k from the neighbouring B row": (_host(pat, A, B_shift), True),
    }


@pytest.mark.parametrize("K", [16, 128, 1024])
@pytest.mark.parametrize("name", ["zipf", "hub"])
def test_ref_agrees_with_the_host_loop(name, K):
    pat = pattern(name)
    A, B = _operands(pat, K, signed_data)
    P, S = sddmm_ref(pat, A, B)
    ratio = bound_ratio(_host(pat, A, B), P, S, K)
    print(f"{name} K={K}: host loop worst |P - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    A, B = _operands(pat, K, grid_data)
    P, S = sddmm_ref(pat, A, B)
    assert np.array_equal(_host(pat, A, B).astype(np.float64), P)
    assert (S >= np.abs(P)).all() and S.max() <= 16.0 * K


@pytest.mark.parametrize("K", KS)
def test_mutations_fail_the_bound_on_signed_data(K):
    pat = pattern("hub")
    A, B = _operands(pat, K, signed_data)
    P, S = sddmm_ref(pat, A, B)
    assert bound_ratio(_host(pat, A, B), P, S, K) <= 1.0
    for what, (Pm, _) in _mutations(pat, A, B).items():
        err = np.abs(Pm.astype(np.float64) - P)
        over = err > sddmm_bound(S, K)
        ratio = bound_ratio(Pm, P, S, K)
        print(f"K={K} {what}: {int(over.sum())} of {len(P)} over the bound, worst {ratio:.1f} x")
        # not one lucky entry: the weakest (fp16 rounding at K = 1024, where the bound's sqrt(K)
        # growth nears fp16's 2^-11 |P|) flags 165 of these 2,176 entries, 2.1 x at the worst
        assert ratio > 1.5 and over.mean() > (0.9 if "k" in what.split() else 0.05), what


@pytest.mark.parametrize("K", KS)
def test_mutations_fail_bit_equality_on_grid_data(K):
    pat = pattern("hub")
    A, B = _operands(pat, K, grid_data)
    P, _ = sddmm_ref(pat, A, B)
    assert np.array_equal(_host(pat, A, B).astype(np.float64), P)
    for what, (Pm, changes) in _mutations(pat, A, B).items():
        differs = int((Pm.astype(np.float64) != P).sum())
        print(f"K={K} {what}: {differs} of {len(P)} differ")
        if changes:  # (fp16 holds multiples of 2^-6 below 32 exactly: at K = 16 few sums exceed it)
            assert differs > len(P) // (20 if "fp16" in what else 2), what
        else:  # 6-bit values have nothing to cut
            assert differs == 0, what


def test_ref_half_operands_and_blocking():
    """Half operands are rounded before the sums, and the entry blocks do not change a value."""
    pat = pattern("empty")
    A, B = _operands(pat, 1024, signed_data)  # 1,107 entries x 1024: one block; K = 16: one block
    for dtype in (F16, BF16):
        P, S = sddmm_ref(pat, A, B, dtype)
        Ah, Bh = half_values(A, dtype), half_values(B, dtype)
        P2, S2 = sddmm_ref(pat, Ah, Bh)
        assert np.array_equal(P, P2) and np.array_equal(S, S2)
        M, N, rp, ci = pat
        e = len(ci) - 1
        r = int(np.searchsorted(rp, e, side="right") - 1)
        want = float(Ah[r].astype(np.float64) @ Bh[ci[e]].astype(np.float64))
        assert P[e] == pytest.approx(want, rel=1e-14)
    big = pattern("zipf")  # 31,170 entries x 1024 = ten blocks
    A, B = _operands(big, 1024, grid_data)
    P, _ = sddmm_ref(big, A, B)
    M, N, rp, ci = big
    for e in (0, 3071, 3072, 3073, len(ci) - 1):
        r = int(np.searchsorted(rp, e, side="right") - 1)
        assert P[e] == float(A[r].astype(np.float64) @ B[ci[e]].astype(np.float64))


def test_grid_data_is_exact_in_every_dtype():
    g = grid_data(100000, 3)
    assert g.dtype == np.float32 and g.min() == -4.0 and g.max() == 3.875
    assert np.array_equal(g * 8, np.round(g * 8)) and len(np.unique(g)) == 64
    for dtype in (F16, BF16):
        assert np.array_equal(half_values(g, dtype), g)
    s = signed_data(100000, 3)
    assert s.dtype == np.float32 and -1.0 <= s.min() and s.max() < 1.0
    assert (half_values(s, F16) != s).mean() > 0.9  # full mantissa: the rounding matters


def test_bound_regimes():
    S = np.array([1.0, 0.0])
    u = 2.0 ** -24
    assert np.allclose(sddmm_bound(S, 4), [8 * u + 1e-6, 1e-6])  # 2 K below K = 16
    assert np.allclose(sddmm_bound(S, 16), [32 * u + 1e-6, 1e-6])  # equal at 16
    assert np.allclose(sddmm_bound(S, 1024), [256 * u + 1e-6, 1e-6])  # 8 sqrt K above
    assert np.allclose(sddmm_bound(S, 64, scale=2.0 ** -24), [64 * u + 1e-6 * u, 1e-6 * u])


def test_case_table_covers_the_dispatch():
    kinds = {c.kind for c in CASES}
    assert kinds == {"colmajor", "half", "rowblock", "dense", "ptile"}
    cm = {c.K for c in CASES if c.kind == "colmajor"}
    assert {16, 48, 32, 96, 64, 128, 256, 512, 192, 1024} <= cm
    for dtype in (F16, BF16):
        assert {32, 96, 128, 512} <= {c.K for c in CASES if c.kind == "half" and c.dtype == dtype}
        assert {rb_slot(c.K, dtype) for c in CASES if c.kind == "rowblock" and c.dtype == dtype} >= {2, 4}
    for half in (False, True):
        slots = {rb_slot(c.K, c.dtype) for c in CASES if c.kind == "rowblock" and (c.dtype != F32) == half}
        assert slots == {0, 1, 2, 3, 4}
    proofs = set().union(*(c.proof for c in CASES if c.kind == "rowblock"))
    assert proofs >= {"rb_pairs", "rb_batches", "rb_orig_rows", "rb_col_blocks", "rb_tiles", "rb_rows", "nt"}
    # pick_rb's product: per dtype 2 workgroup sizes x (5 sizes x {lite, full} + 3 x 2 with batches
    # + 3 paired + 1 paired with batches)
    for dtype in (F32, F16, BF16):
        assert sum(c.name.startswith("rbx_") and c.dtype == dtype for c in CASES) == 2 * (10 + 6 + 3 + 1)
    knobs = set().union(*(c.tuning for c in CASES))
    assert knobs >= {"out_staged", "pair_min_items", "batches", "orig_rows", "col_blocks", "tile_min_f32",
                     "tile_min_half", "l2_range_kb", "rb_rows", "dense_ks", "dense_ns", "ptile"}
    for dtype in (F16, BF16):  # k_sddmm_dense: every ring depth at eight waves, four waves at NS = 2
        dense = [c for c in CASES if c.kind == "dense" and c.dtype == dtype]
        assert {c.tuning.get("dense_ns", 2) for c in dense if "dense_ks" not in c.tuning} == {2, 3, 4, 5}
        assert {c.K for c in dense if c.tuning.get("dense_ks") == 1} == {64, 320}
        # k_sddmm_ptile: every K at four waves (tpi <= 4) and eight, items past the wave count,
        # two-panel runs
        pt = [c for c in CASES if c.kind == "ptile" and c.dtype == dtype]
        for tpi in (3, 8, 64, 0):
            assert {c.K for c in pt if c.tuning.get("ptile_tpi", 0) == tpi and c.proof} == {64, 128, 256, 512}
        assert {c.K for c in pt if c.proof.get("ptile_two_panels")} == {64, 128, 256, 512}
        assert max(c.proof.get("ptile_max_tiles", 0) for c in pt) > 8
    # k_sddmm_panels_f32<KT, G>: the K of every reachable (KT, G)
    assert {BY_NAME[n].K for n in PANEL_CASES if BY_NAME[n].kind == "colmajor"} == \
        {16, 48, 96, 32, 64, 128, 256, 512, 192, 1024}
    assert {(c.pattern, c.K) for c in CASES if c.kind == "dense"} >= {("uniform300", 64), ("uniform300", 320)}
    assert {(c.pattern, c.K) for c in CASES if c.kind == "ptile"} >= {("blockmask", 64), ("blockmask", 512)}
    assert {BY_NAME[n].kind for n in ONE_PER_KIND} == kinds
    assert all(n in BY_NAME for n in PANEL_CASES)
    for c in CASES:  # the suite's small patterns only (the larger: test_gpu_ptile's 768 x 768 mask)
        assert len(pattern(c.pattern)[3]) <= (42000 if c.pattern != "blockmask768" else 120000)
    assert pattern("zipf")[0] % 16 != 0
    M, N, rp, ci = pattern("empty")
    assert (np.diff(rp.astype(np.int64)) == 0).any() and len(np.unique(ci)) < N


@pytest.mark.parametrize("nnz", [0, 1])
def test_plan_create_rejects_fewer_than_two_entries(nnz):
    """include/bsmr.h bsmr_plan_create: nnz >= 2, refused before any device call."""
    rp = np.array([0, nnz, nnz], np.uint32)
    ci = np.zeros(nnz, np.uint32)
    with pytest.raises(bsmr.BsmrError) as ei:
        bsmr.Plan(2, 3, rp, ci)
    assert ei.value.status == 1  # BSMR_ERR_INVALID
    assert "nnz >= 2" in str(ei.value)


def _plan_status(M, N, rp, ci):
    """(status, message) of bsmr_plan_create on the host CSR; (0, "") when a plan was built."""
    try:
        bsmr.Plan(M, N, np.asarray(rp, np.uint32), np.asarray(ci, np.uint32))
    except bsmr.BsmrError as e:
        return e.status, str(e)
    return 0, ""


# 3 rows, N = 8, 6 entries; each case breaks one rule of the CSR contract (include/bsmr.h)
@pytest.mark.parametrize("rp,ci,N,needle", [
    ([0, 4, 2, 6], [0, 1, 2, 3, 4, 5], 8, "rowptr decreases at row 1"),
    ([0, 7, 6, 6], [0, 1, 2, 3, 4, 5], 8, "rowptr decreases at row 1"),   # rowptr[1] > nnz as well
    ([1, 2, 4, 6], [0, 1, 2, 3, 4, 5], 8, "rowptr[0] = 1"),
    ([0, 2, 4, 6], [0, 1, 2, 3, 8, 5], 8, "colidx[4] = 8 >= N = 8"),
    ([0, 2, 4, 6], [0, 1, 2, 3, 4, 2 ** 32 - 1], 8, "colidx[5] = 4294967295 >= N = 8"),
    ([0, 2, 4, 6], [0, 9, 2, 3, 8, 5], 8, "colidx[1] = 9"),               # the first offender
])
def test_plan_create_rejects_invalid_csr(rp, ci, N, needle):
    """include/bsmr.h bsmr_plan_create: rowptr[0] == 0, rowptr non-decreasing, colidx < N; refused
    with BSMR_ERR_INVALID and the first offending row or entry, before any device call (a column
    block index past the row's LDS histogram would otherwise be written by k_encode)."""
    st, msg = _plan_status(3, N, rp, ci)
    assert st == 1, (st, msg)  # BSMR_ERR_INVALID
    assert "bsmr_plan_create" in msg and needle in msg, msg


@pytest.mark.parametrize("rp,ci,needle", [
    ([0, 4, 2, 6], [0, 1, 2, 3, 4, 5], "rowptr decreases at row 1"),
    ([1, 2, 4, 6], [0, 1, 2, 3, 4, 5], "rowptr[0] = 1"),
    ([0, 2, 4, 6], [0, 1, 2, 3, 8, 5], "colidx[4] = 8 >= N = 8"),
    ([0, 2, 4, 6], [0, 1, 2, 3, 4, 2 ** 32 - 1], "colidx[5] = 4294967295"),
])
def test_plan_import_rows_rejects_invalid_csr(rp, ci, needle):
    """bsmr_plan_import_rows applies the same CSR contract before its own header checks and before
    any device call."""
    hdr = bsmr.RowStage(M=3, N=8, nnz=6, block_size=16, num_blocks_per_row=1, cluster_block_dim=32,
                        num_zero_rows=0, num_reordered_rows=3, num_clusters=1, alpha=0.3)
    with pytest.raises(bsmr.BsmrError) as ei:
        bsmr.Plan.from_row_stage(np.asarray(rp, np.uint32), np.asarray(ci, np.uint32), hdr,
                                 np.arange(3, dtype=np.uint32))
    assert ei.value.status == 1, str(ei.value)
    assert "bsmr_plan_import_rows" in str(ei.value) and needle in str(ei.value), str(ei.value)


def test_plan_create_accepts_unsorted_columns_up_to_the_device_step():
    """A legal CSR whose columns are not sorted inside a row (the loaders keep file order) passes
    the host validation: the call gets as far as the device (BSMR_ERR_HIP without one, a plan
    with one), never BSMR_ERR_INVALID."""
    st, msg = _plan_status(3, 8, [0, 2, 4, 6], [7, 0, 3, 2, 5, 1])
    assert st in (0, 4), (st, msg)  # BSMR_OK or BSMR_ERR_HIP
    if st == 4:
        assert "hip" in msg.lower(), msg
