"""CPU: tests/attention_cases.py checked against itself, so that the GPU tests of the fused sparse
attention forward stand on a reference, bounds and data sets that are known to tell a right kernel
from a subtly wrong one.

* the numpy-fp32 emulation of the documented summation order (attention_emulate over the library's
  own bsmr.spmm_lists) stays inside attention_bound / lse_bound on every pattern and signed data set
  of the GPU tests, and reproduces the selector data bit for bit; the worst ratios are printed;
* every mutation of the emulation fails at least one of those checks; `partial_not_rescaled` and
  `max_without_last_segment` are caught by the ascending selector data (the maximum grows in every
  segment): a common reference other than the maximum is harmless in exact arithmetic, so bounded
  random data does not show it;
* the bounds are those the module derives: the attention constant is softmax_cases' plus 3, the
  list parameters come from bsmr.attention_limits().
"""
import functools

import numpy as np
import pytest

import attention_cases as AC
import bsmr
import softmax_cases as SC
from bsmr import BF16, F32

CPU_SHAPES = [(F32, 32, 48), (BF16, 64, 64)]  # the generic form with D != Dv; a compile-time form
SIGNED = [("narrow", 1.0), ("wide", 0.125), ("wide", None)]  # None: 1 / sqrt(D)


def test_constants_come_from_the_library():
    lim = AC.limits()
    assert lim == bsmr.attention_limits() and lim["chunk"] % 64 == 0 and lim["max_row_bytes"] == 1024
    assert AC.C_ATTN == SC.C_FWD + 3
    lens = AC.row_lengths(AC.pattern("long4"))
    assert lens.max() == 4 * lim["chunk"] + 3
    for n in (0, 1, lim["chunk"] - 1, lim["chunk"], lim["chunk"] + 1, 2 * lim["chunk"], 2 * lim["chunk"] + 1):
        assert (lens == n).any(), n
    assert set(range(272)) <= set(AC.row_lengths(AC.pattern("staircase")).tolist())


def test_lane_forms():
    assert AC.lane_form(16, 16, F32) == (4, 4, 4, 4)
    assert AC.lane_form(32, 48, F32) == (16, 4, 8, 12)
    assert AC.lane_form(48, 128, F32) == (32, 4, 12, 32)
    assert AC.lane_form(256, 256, F32) == (64, 4, 64, 64)
    assert AC.lane_form(32, 128, BF16) == (16, 8, 4, 16)
    assert AC.lane_form(512, 512, BF16) == (64, 8, 64, 64)


@pytest.mark.parametrize("dtype,D,Dv", CPU_SHAPES, ids=lambda x: str(x))
@pytest.mark.parametrize("name", AC.PATTERNS)
def test_emulation_stays_inside_the_bound(name, dtype, D, Dv):
    pat = AC.pattern(name)
    for kind, scale in SIGNED:
        scale = D ** -0.5 if scale is None else scale
        Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, kind, scale)
        ref = AC.attention_ref(pat, Q, K, V, scale, dtype)
        O, LSE = AC.attention_emulate(pat, Q, K, V, scale, dtype)
        top = np.abs(ref["d"]).max() if len(ref["d"]) else 0.0
        print(f"largest |d| = {top:.2f}")
        AC.check_bound(O, LSE, ref, f"emulation {name} {kind} scale {scale:.4f} {AC.DTYPE_NAME[dtype]} {D}x{Dv}", opscale)


@pytest.mark.parametrize("dtype,D,Dv", CPU_SHAPES, ids=lambda x: str(x))
@pytest.mark.parametrize("name", AC.PATTERNS)
def test_emulation_reproduces_the_selector_data(name, dtype, D, Dv):
    pat = AC.pattern(name)
    for order in ("random", "ascending", "descending"):
        Q, K, V, winner, pi, base = AC.selector(pat, D, Dv, order, dtype)
        for scale in AC.SCALES_EXACT:
            O, LSE = AC.attention_emulate(pat, Q, K, V, scale, dtype)
            wantO, wantL = AC.selector_expected(V, winner, pi, base, scale, dtype)
            AC.check_exact(O, wantO, f"O {name} {order} {scale}")
            AC.check_exact(LSE, wantL, f"LSE {name} {order} {scale}")


def test_the_reference_is_the_dense_masked_attention():
    pat = AC.pattern("empty")
    M, N, rp, ci = pat
    D, Dv, scale = 16, 32, 0.25
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "wide", scale)
    ref = AC.attention_ref(pat, Q, K, V, scale)
    mask = np.zeros((M, N), bool)
    mask[AC.entry_rows(pat), np.asarray(ci, np.int64)] = True
    S = np.where(mask, Q.astype(np.float64) @ K.astype(np.float64).T * scale, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        mx = np.where(mask.any(axis=1), S.max(axis=1), 0.0)
        T = np.exp(S - mx[:, None])
        den = T.sum(axis=1)
        O = (T / np.where(den == 0, 1.0, den)[:, None]) @ V.astype(np.float64)
        LSE = np.where(den == 0, -np.inf, mx + np.log(den))
    assert np.abs(O - ref["O"]).max() < 1e-13
    live = den > 0
    assert np.abs(LSE[live] - ref["LSE"][live]).max() < 1e-12 and (ref["LSE"][~live] == -np.inf).all()
    assert (ref["O"][~live] == 0).all()


@functools.lru_cache(maxsize=None)
def _mutation_checks(mutation):
    """{check name: failed} of one mutation over the split-row patterns."""
    out = {}
    dtype, D, Dv = F32, 32, 48
    for name in ("staircase", "long4"):
        pat = AC.pattern(name)
        for order in ("ascending", "random"):
            Q, K, V, winner, pi, base = AC.selector(pat, D, Dv, order, dtype)
            O, LSE = AC.attention_emulate(pat, Q, K, V, 0.125, dtype, mutation)
            wantO, wantL = AC.selector_expected(V, winner, pi, base, 0.125, dtype)
            try:
                AC.check_exact(O, wantO, "O")
                AC.check_exact(LSE, wantL, "LSE")
                out[f"{name}/{order}"] = False
            except AssertionError:
                out[f"{name}/{order}"] = True
        Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, "narrow", 1.0)
        ref = AC.attention_ref(pat, Q, K, V, 1.0, dtype)
        O, LSE = AC.attention_emulate(pat, Q, K, V, 1.0, dtype, mutation)
        ro, rl = AC.bound_ratios(O, LSE, ref, opscale)
        out[f"{name}/signed"] = not (ro <= 1.0 and rl <= 1.0)
    return out


@pytest.mark.parametrize("mutation", AC.MUTATIONS)
def test_every_mutation_fails_a_check(mutation):
    failed = _mutation_checks(mutation)
    print(mutation, failed)
    assert any(failed.values()), f"{mutation} passes every check"
    if mutation in ("partial_not_rescaled", "max_without_last_segment"):
        assert failed["staircase/ascending"] and failed["long4/ascending"], (mutation, failed)


def test_the_unmutated_emulation_passes_those_checks():
    assert not any(_mutation_checks(None).values())
