"""CPU: the checker of the SpMM / SDDMM-gradient tests checks itself (tests/spmm_cases.py).

* spmm_emulate (the kernel's documented summation order in numpy fp32 over the library's host
  lists) equals spmm_ref (float64) bit for bit on grid data: `staircase`, `hub` and `zipf`, both
  sides, chunk 1, 32, 64, 65, 128 and 1 << 20, lane counts L = 2, 8 and 64. This is the exactness
  argument of grid data, run: no chunk, lane group, butterfly or reduce order rounds.
* On signed data the emulation stays within signed_bound_tight (worst ratio printed per pattern
  and side).
* Five mutations of the emulation (a segment's last entry dropped, an overlapping chunk boundary,
  vpos shifted by one inside a list, the last partial row left out of the reduce, the result
  rounded to bf16) each fail bit equality on grid data at exactly the destinations they touch,
  and on signed data put at least one element of every touched destination with n >= 2 over the
  tight bound, while every untouched destination stays exact / within it. This pins the checks:
  a bound loose enough to pass one of them fails here.
* The tight bound's regimes; grid and signed values; the staircase's list lengths; the stats the
  GPU tests expect against the library's own lists; SPMM_CASES reaches every instantiation.
"""
import numpy as np
import pytest

import bsmr
from bsmr import BF16, F16, F32
from gpu_util import half_values
from sddmm_cases import grid_data, signed_data
from spmm_cases import (MUTATIONS, SPMM_CASES, SPMM_DIRECT, bound_ratio, expected_stats, grid_values, list_lengths,
                        mutation_touches, pattern, row_bytes, signed_bound, signed_bound_tight, signed_values,
                        spmm_emulate, spmm_form, spmm_ref)

KX = 16  # columns of X: the summation order depends on the row size handed to spmm_emulate alone
CHUNKS = [1, 32, 64, 65, 128, 1 << 20]
ROW_BYTES = [32, 96, 1024]  # L = 2, 8 (6 live), 64


def _operands(pat, side, data):
    M, N, _, ci = pat
    rows = N if side == 1 else M
    if data == "grid":
        return grid_values(len(ci), 21), grid_data(rows * KX, 22 + side).reshape(rows, KX)
    return signed_values(len(ci), 31), signed_data(rows * KX, 32 + side).reshape(rows, KX)


@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("name", ["staircase", "hub", "zipf"])
def test_emulation_is_exact_on_grid_data_and_bounded_on_signed(name, side):
    pat = pattern(name)
    V, X = _operands(pat, side, "grid")
    ref = spmm_ref(pat, side, V, X)
    assert np.abs(ref[0]).max() <= 16.0 * ref[2].max() < 2.0 ** 18
    Vs, Xs = _operands(pat, side, "signed")
    refs = spmm_ref(pat, side, Vs, Xs)
    worst = 0.0
    for chunk in CHUNKS:
        for rb in ROW_BYTES:
            Y = spmm_emulate(pat, side, chunk, V, X, rb)
            assert Y.dtype == np.float32 and np.isfinite(Y).all()
            assert np.array_equal(Y.astype(np.float64), ref[0]), (name, side, chunk, rb)
            worst = max(worst, bound_ratio(spmm_emulate(pat, side, chunk, Vs, Xs, rb), refs))
    print(f"RATIO spmm/emulation {worst:.4f} {name} side {side}")
    assert worst <= 1.0


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("name", ["staircase", "hub"])
def test_mutations_are_rejected(name, side, mutation):
    pat = pattern(name)
    n = list_lengths(pat, side)
    rb = 128  # L = 8: eight lane groups and the butterfly
    touched_any = False
    for chunk in (32, 128):
        # grid data: bit equality fails at exactly the touched destinations
        V, X = _operands(pat, side, "grid")
        ref = spmm_ref(pat, side, V, X)
        touched = mutation_touches(pat, side, chunk, V, ref, mutation)
        Y = spmm_emulate(pat, side, chunk, V, X, rb, mutation=mutation)
        differs = (Y.astype(np.float64) != ref[0]).any(axis=1)
        slipped = np.nonzero(touched & ~differs)[0]
        assert len(slipped) == 0, (f"{mutation} chunk {chunk}: passes bit equality at destinations "
                                   f"{slipped[:8]} (lists of {n[slipped[:8]]})")
        assert not (differs & ~touched).any(), f"{mutation} chunk {chunk}: changes an untouched destination"
        # signed data: every touched destination with n >= 2 has an element over the tight bound
        V, X = _operands(pat, side, "signed")
        ref = spmm_ref(pat, side, V, X)
        touched = mutation_touches(pat, side, chunk, V, ref, mutation) & (n >= 2)
        Y = spmm_emulate(pat, side, chunk, V, X, rb, mutation=mutation)
        over = (np.abs(Y.astype(np.float64) - ref[0]) > signed_bound_tight(ref[1], ref[2])).any(axis=1)
        slipped = np.nonzero(touched & ~over)[0]
        assert len(slipped) == 0, (f"{mutation} chunk {chunk}: within the tight bound at destinations "
                                   f"{slipped[:8]} (lists of {n[slipped[:8]]})")
        assert not (over & ~touched & (n >= 2)).any(), f"{mutation} chunk {chunk}: an untouched destination is over"
        print(f"{name} side {side} {mutation} chunk {chunk}: {int(differs.sum())} destinations differ on grid "
              f"data, {int(touched.sum())} with n >= 2 over the bound on signed data")
        touched_any |= bool(touched.any())
    # (the hub pattern's columns hold at most four entries: no list of theirs is split)
    assert touched_any or (name == "hub" and side == 2 and mutation in ("double_first", "skip_last_partial"))


def test_the_older_bound_passes_a_dropped_term_the_tight_one_rejects():
    """The hub row (n = 2048) with a standard normal V, as tests/test_gpu_spmm.py draws it: its last
    term dropped stays inside 2 n 2^-24 S in every column and over the tight bound in most."""
    pat = pattern("hub")
    M, N, rp, ci = pat
    K = 128
    V = np.random.default_rng(17).standard_normal(len(ci)).astype(np.float32)
    X = signed_data(N * K, 5).reshape(N, K)
    Yr, S, n = spmm_ref(pat, 1, V, X)
    hub = int(n.argmax())
    assert n[hub] == 2048
    Y = spmm_emulate(pat, 1, 1 << 20, V, X, 512)
    e = int(rp[hub + 1]) - 1  # the hub row's last entry
    Y[hub] -= V[e] * X[ci[e]]
    err = np.abs(Y[hub].astype(np.float64) - Yr[hub])
    loose = int((err <= signed_bound(S, n)[hub]).sum())
    tight = int((err <= signed_bound_tight(S, n)[hub]).sum())
    print(f"dropped last term of the hub row: inside the older bound in {loose} of {K} columns, "
          f"inside the tight bound in {tight}")
    assert loose > tight and tight < K // 2  # (this V's last value is small: 128 and 17)


def test_bound_regimes():
    S = np.array([[1.0, 0.0]] * 3)
    n = np.array([4, 16, 1024])
    u = 2.0 ** -24
    b = signed_bound_tight(S, n)
    assert np.allclose(b[:, 0], [8 * u + 1e-6, 32 * u + 1e-6, 256 * u + 1e-6], rtol=1e-12)  # 2 n, equal, 8 sqrt n
    assert np.allclose(b[:, 1], 1e-6)
    assert (b <= signed_bound(S, n)).all()
    assert np.allclose(signed_bound_tight(S, n, scale=u)[:, 1], 1e-6 * u)
    assert np.array_equal(signed_bound_tight(np.zeros((1, 2)), np.array([0])), [[1e-6, 1e-6]])  # an empty list


def test_values():
    g = grid_values(100000, 3)
    assert g.dtype == np.float32 and g.min() == -4.0 and g.max() == 3.875 and (g != 0).all()
    assert np.array_equal(g * 8, np.round(g * 8)) and len(np.unique(g)) == 63
    for dtype in (F16, BF16):
        assert np.array_equal(half_values(g, dtype), g)
    s = signed_values(100000, 3)
    assert s.dtype == np.float32 and 0.5 <= np.abs(s).min() and np.abs(s).max() < 1.5
    assert 0.45 < (s > 0).mean() < 0.55 and len(np.unique(s)) > 90000


def test_staircase_holds_every_list_length():
    pat = pattern("staircase")
    M, N, rp, ci = pat
    assert M == N == 272 and len(ci) == 36856
    assert np.array_equal(list_lengths(pat, 1), np.arange(272))
    assert np.array_equal(list_lengths(pat, 2), 271 - np.arange(272))
    # every segment count 1 .. chunk, with remainders of every size after one and two full chunks
    for chunk in (32, 128):
        for side in (1, 2):
            segs, _, _ = bsmr.spmm_lists(M, N, rp, ci, side, chunk)
            assert set(segs[:, 2]) == set(range(chunk + 1))
    rem = {(n // 128, n % 128) for n in range(272)}
    assert {(1, r) for r in range(128)} <= rem and {(2, r) for r in range(16)} <= rem


@pytest.mark.parametrize("name", ["staircase", "hub", "zipf", "empty"])
def test_expected_stats_match_the_library_lists(name):
    pat = pattern(name)
    M, N, rp, ci = pat
    for side in (1, 2):
        for chunk in CHUNKS:
            segs, _, _ = bsmr.spmm_lists(M, N, rp, ci, side, chunk)
            st = expected_stats(pat, side, chunk)
            split = segs[:, 3] != SPMM_DIRECT
            assert st["segments"] == len(segs) and st["partials"] == int(split.sum())
            assert st["split_dsts"] == len(np.unique(segs[split, 0]))
            assert st["max_list"] == int(list_lengths(pat, side).max())
    st = expected_stats(pattern("hub"), 1, 1 << 20)
    assert st["split_dsts"] == 0 and st["max_list"] == 2048 and st["segments"] == 67


def test_case_table_reaches_every_instantiation():
    forms = {(K, dtype): spmm_form(K, dtype) for K, dtype in SPMM_CASES}
    assert len(forms) == len(SPMM_CASES)
    for dtype in (F32, F16, BF16):
        mine = {kd: f for kd, f in forms.items() if kd[1] == dtype}
        fixed = {(f["lanes"], f["ch"]): row_bytes(*kd) for kd, f in mine.items() if f["fixed"]}
        assert fixed == {(8, 1): 128, (16, 1): 256, (32, 1): 512, (64, 1): 1024, (64, 2): 2048}
        generic = [f for f in mine.values() if not f["fixed"]]
        lanes = {f["lanes"] for f in generic if f["tiles"] == 1}
        assert lanes >= ({4, 16, 32, 64} if dtype == F32 else {2, 4, 8, 16, 32, 64})  # (32 B, 96 B: halves only)
        assert {f["tiles"] for f in generic} >= ({1, 2, 3, 4} if dtype == F32 else {1, 2, 3})
    generic = {row_bytes(*kd): f for kd, f in forms.items() if not f["fixed"]}
    assert set(generic) == {32, 64, 96, 192, 384, 768, 1280, 3072, 4096}
    assert {f["lanes"] for f in generic.values()} == {2, 4, 8, 16, 32, 64}
    assert {f["tiles"] for f in generic.values()} == {1, 2, 3, 4}
    assert (generic[96]["lanes"], generic[96]["live"]) == (8, 6)
    assert (generic[384]["lanes"], generic[384]["live"]) == (32, 24)
    assert (generic[768]["lanes"], generic[768]["live"]) == (64, 48)
    assert (generic[1280]["tiles"], generic[1280]["live"]) == (2, 16)
    assert (generic[4096]["tiles"], generic[4096]["live"]) == (4, 64)
    assert sum(f["fixed"] for f in forms.values()) == 15
    assert max(K * 2 for K, dtype in SPMM_CASES if dtype != F32) == 3072
