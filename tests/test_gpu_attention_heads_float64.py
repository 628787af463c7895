"""GPU: the fused sparse attention over batch and heads (bsmr_attention_heads,
bsmr_attention_backward_heads) against the existing single-slice calls and the float64 answer.

Data chosen to show cross-talk (tests/attention_heads_cases.py): every slice has its own seed, so
the selector data has other winners and the signed data other values in every slice. Patterns:
long4 (split rows: per-slice scratch can only go wrong with two slices and a split row), hub (a
2048-entry row), empty (empty rows); the backward also long4_T and hub_T (split columns). Shapes:
one generic and one compile-time lane form per dtype. (B, H) = (1, 3) and (2, 2); layouts dense
bhmd, bmhd (head stride D, row stride H D), bhmd with a padded row stride, K / V with head stride 0.

  1. forward and backward outputs of every slice are bit for bit those of the existing single-slice
     call on a contiguous copy (attention_cases.attention_once, attention_bwd_cases.backward_once);
  2. selector and flat data are bit for bit the float64 answer, directly (not through 1);
  3. signed data per dtype inside attention_bound / backward_bound per slice ("RATIO ..." lines).

Also bit for bit, with no tolerance: two launches of the same call; a lazily built plan against a
prepared plan; LSE pointer given or NULL; each NULL-output combination of the backward against the
full call; a single-slice launch between two heads launches; B = H = 1 with dense strides against
bsmr_attention and bsmr_attention_backward.
"""
import itertools

import numpy as np
import pytest

import attention_bwd_cases as BC
import attention_cases as AC
import attention_heads_cases as HC
from bsmr import F16, F32

pytestmark = pytest.mark.gpu
S_SIGNED, S_EXACT = 0.25, 0.125
SHAPE_IDS = [f"{HC.DTYPE_NAME[t]}_{D}x{Dv}" for t, D, Dv in HC.SHAPES]
BH_IDS = [f"B{b}H{h}" for b, h in HC.BH]


def _fwd_slices(kind, name, D, Dv, dtype, scale, B, H, layout):
    return [HC.forward_slice(kind, name, D, Dv, dtype, scale, sq, skv) for sq, skv in HC.seeds(B, H, layout)]


def _bwd_slices(kind, name, D, Dv, dtype, scale, B, H, layout):
    return [HC.backward_slice(kind, name, D, Dv, dtype, scale, sq, skv) for sq, skv in HC.seeds(B, H, layout)]


@pytest.mark.parametrize("layout", HC.LAYOUTS)
@pytest.mark.parametrize("bh", HC.BH, ids=BH_IDS)
@pytest.mark.parametrize("shape", HC.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", HC.FWD_PATTERNS)
def test_forward_slices(name, shape, bh, layout):
    dtype, D, Dv = shape
    B, H = bh
    plan = HC.plan_of(name)
    pat = BC.pattern(name)
    what = f"{name} {HC.DTYPE_NAME[dtype]} {D}x{Dv} B{B} H{H} {layout}"
    # 1. signed data against the single-slice call
    sl = _fwd_slices("signed", name, D, Dv, dtype, S_SIGNED, B, H, layout)
    O, L = HC.heads_forward_once(plan, sl, B, H, layout, S_SIGNED, dtype)
    single = [HC.single_forward(name, D, Dv, dtype, S_SIGNED, sq, skv) for sq, skv in HC.seeds(B, H, layout)]
    HC.assert_slices_equal(O, [s[0] for s in single], f"O signed {what}")
    HC.assert_slices_equal(L[:, :, None], [s[1][:, None] for s in single], f"LSE signed {what}")
    # 3. inside the bound per slice (one (B, H) and layout per pattern and shape)
    if bh == HC.BH[0] and layout == "bhmd":
        for z, s in enumerate(sl):
            AC.check_bound(O[z], L[z], AC.attention_ref(pat, s["Q"], s["K"], s["V"], S_SIGNED, dtype),
                           f"heads {what} slice {z}", s["opscale"])
    # 2. selector data against the float64 answer
    sl = _fwd_slices("selector", name, D, Dv, dtype, S_EXACT, B, H, layout)
    O, L = HC.heads_forward_once(plan, sl, B, H, layout, S_EXACT, dtype)
    HC.assert_slices_equal(O, [s["O"] for s in sl], f"O selector {what}")
    HC.assert_slices_equal(L[:, :, None], [s["LSE"][:, None] for s in sl], f"LSE selector {what}")
    if H > 1 and layout != "kv_shared" and name != "empty":
        assert not HC.bits_equal(O[0], O[1]), "two slices with their own data gave equal outputs"


@pytest.mark.parametrize("layout", HC.LAYOUTS)
@pytest.mark.parametrize("bh", HC.BH, ids=BH_IDS)
@pytest.mark.parametrize("shape", HC.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", HC.BWD_PATTERNS)
def test_backward_slices(name, shape, bh, layout):
    dtype, D, Dv = shape
    B, H = bh
    plan = HC.plan_of(name)
    pat = BC.pattern(name)
    what = f"{name} {HC.DTYPE_NAME[dtype]} {D}x{Dv} B{B} H{H} {layout}"
    # 1. signed data against the single-slice call
    sl = _bwd_slices("signed", name, D, Dv, dtype, S_SIGNED, B, H, layout)
    got = HC.heads_backward_once(plan, sl, B, H, layout, S_SIGNED, dtype)
    single = [HC.single_backward(name, D, Dv, dtype, S_SIGNED, sq, skv) for sq, skv in HC.seeds(B, H, layout)]
    for k in HC.OUTPUTS:
        HC.assert_slices_equal(got[k], [s[k] for s in single], f"{k} signed {what}")
    # 3. inside the bound per slice
    if bh == HC.BH[0] and layout == "bhmd":
        for z, s in enumerate(sl):
            ref = BC.backward_ref(pat, s["Q"], s["K"], s["V"], s["O"], s["GO"], s["LSE"], S_SIGNED, dtype)
            BC.check_bound({k: got[k][z] for k in HC.OUTPUTS}, ref, f"heads {what} slice {z}", s["opscale"])
    # 2. both exact sets against the float64 answer
    for kind in ("selector", "flat"):
        sl = _bwd_slices(kind, name, D, Dv, dtype, S_EXACT, B, H, layout)
        got = HC.heads_backward_once(plan, sl, B, H, layout, S_EXACT, dtype)
        for k in HC.OUTPUTS:
            HC.assert_slices_equal(got[k], [s[k] for s in sl], f"{k} {kind} {what}")


# ----------------------------------------------------------------- bit for bit, no tolerance ----
CASES = [("long4", F32, 32, 48, 2, 2, "bmhd"), ("long4_T", F16, 64, 64, 1, 3, "padded")]
CASE_IDS = [f"{c[0]}_{HC.DTYPE_NAME[c[1]]}_{c[6]}" for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_repeat_lazy_prepared_and_lse_pointer(case):
    name, dtype, D, Dv, B, H, layout = case
    Z = B * H
    fs = _fwd_slices("signed", name, D, Dv, dtype, S_SIGNED, B, H, layout)
    bs = _bwd_slices("signed", name, D, Dv, dtype, S_SIGNED, B, H, layout)
    lazy, prepared = BC.make_plan(BC.pattern(name)), BC.make_plan(BC.pattern(name))
    prepared.prepare_attention_heads(D, Dv, Z)
    prepared.prepare_attention_backward_heads(D, Dv, Z)
    assert prepared.attention_heads_prepared(D, Dv, Z) and prepared.attention_backward_heads_prepared(D, Dv, Z)
    assert not lazy.attention_heads_prepared(D, Dv, 1) and not lazy.attention_backward_heads_prepared(D, Dv, 1)
    O1, L1 = HC.heads_forward_once(lazy, fs, B, H, layout, S_SIGNED, dtype)
    assert lazy.attention_heads_prepared(D, Dv, Z)
    O2, L2 = HC.heads_forward_once(lazy, fs, B, H, layout, S_SIGNED, dtype)
    O3, L3 = HC.heads_forward_once(prepared, fs, B, H, layout, S_SIGNED, dtype)
    O4, L4 = HC.heads_forward_once(prepared, fs, B, H, layout, S_SIGNED, dtype, lse=False)
    assert HC.bits_equal(O1, O2) and HC.bits_equal(L1, L2), "two launches of the same call differ"
    assert HC.bits_equal(O1, O3) and HC.bits_equal(L1, L3), "a lazily built and a prepared plan differ"
    assert HC.bits_equal(O1, O4) and L4 is None, "O depends on whether LSE is asked for"
    g1 = HC.heads_backward_once(lazy, bs, B, H, layout, S_SIGNED, dtype)
    assert lazy.attention_backward_heads_prepared(D, Dv, Z)
    g2 = HC.heads_backward_once(lazy, bs, B, H, layout, S_SIGNED, dtype)
    g3 = HC.heads_backward_once(prepared, bs, B, H, layout, S_SIGNED, dtype)
    for k in HC.OUTPUTS:
        assert HC.bits_equal(g1[k], g2[k]), f"two launches of the same call differ in {k}"
        assert HC.bits_equal(g1[k], g3[k]), f"a lazily built and a prepared plan differ in {k}"
    # the scratch is what the header promises, per slice, in bytes allocated
    st = prepared.attention_backward_stats()
    assert st["delta_bytes"] == 4 * Z * prepared.M
    assert st["row_scratch_bytes"] == 4 * Z * st["row_partials"] * D
    assert st["col_scratch_bytes"] == 4 * Z * st["col_partials"] * (D + Dv)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_null_output_combinations(case):
    name, dtype, D, Dv, B, H, layout = case
    plan = HC.plan_of(name)
    bs = _bwd_slices("signed", name, D, Dv, dtype, S_SIGNED, B, H, layout)
    dev = HC.backward_inputs(bs, B, H, layout, dtype)
    full = HC.heads_backward_once(plan, bs, B, H, layout, S_SIGNED, dtype, dev=dev)
    for n in (1, 2):
        for want in itertools.combinations(HC.OUTPUTS, n):
            got = HC.heads_backward_once(plan, bs, B, H, layout, S_SIGNED, dtype, want=want, dev=dev)
            for k in HC.OUTPUTS:
                if k in want:
                    assert HC.bits_equal(got[k], full[k]), f"{k} of {want} differs from the full call"
                else:
                    assert got[k] is None


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_single_slice_launch_between_two_heads_launches(case):
    name, dtype, D, Dv, B, H, layout = case
    plan = HC.plan_of(name)
    fs = _fwd_slices("signed", name, D, Dv, dtype, S_SIGNED, B, H, layout)
    bs = _bwd_slices("signed", name, D, Dv, dtype, S_SIGNED, B, H, layout)
    other = HC.SEED0 + HC.SEED_STEP * 9
    f1 = HC.forward_slice("signed", name, D, Dv, dtype, S_SIGNED, other, other)
    b1 = HC.backward_slice("signed", name, D, Dv, dtype, S_SIGNED, other, other)
    O1, L1 = HC.heads_forward_once(plan, fs, B, H, layout, S_SIGNED, dtype)
    Os, Ls = AC.attention_once(plan, f1["Q"], f1["K"], f1["V"], S_SIGNED, dtype)
    O2, L2 = HC.heads_forward_once(plan, fs, B, H, layout, S_SIGNED, dtype)
    assert HC.bits_equal(O1, O2) and HC.bits_equal(L1, L2)
    fresh = BC.make_plan(BC.pattern(name))  # a plan that only ever sees single-slice calls
    Of, Lf = AC.attention_once(fresh, f1["Q"], f1["K"], f1["V"], S_SIGNED, dtype)
    assert HC.bits_equal(Os, Of) and HC.bits_equal(Ls, Lf), "a single-slice call changed after a heads call"
    g1 = HC.heads_backward_once(plan, bs, B, H, layout, S_SIGNED, dtype)
    gs = BC.backward_once(plan, b1["Q"], b1["K"], b1["V"], b1["O"], b1["GO"], b1["LSE"], S_SIGNED, dtype)
    g2 = HC.heads_backward_once(plan, bs, B, H, layout, S_SIGNED, dtype)
    gf = BC.backward_once(fresh, b1["Q"], b1["K"], b1["V"], b1["O"], b1["GO"], b1["LSE"], S_SIGNED, dtype)
    assert BC.same_bits(gs, gf), "a single-slice backward changed after a heads call"
    for k in HC.OUTPUTS:
        assert HC.bits_equal(g1[k], g2[k])
    # the fresh plan's stats are those of single-slice calls alone
    assert fresh.attention_backward_stats() == BC.expected_stats(BC.pattern(name), D, Dv)


@pytest.mark.parametrize("shape", HC.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", ["long4", "hub_T"])
def test_one_slice_dense_is_the_existing_call(name, shape):
    dtype, D, Dv = shape
    sq = HC.SEED0
    f = HC.forward_slice("signed", name, D, Dv, dtype, S_SIGNED, sq, sq)
    b = HC.backward_slice("signed", name, D, Dv, dtype, S_SIGNED, sq, sq)
    heads, single = BC.make_plan(BC.pattern(name)), BC.make_plan(BC.pattern(name))
    O, L = HC.heads_forward_once(heads, [f], 1, 1, "bhmd", S_SIGNED, dtype)
    Os, Ls = AC.attention_once(single, f["Q"], f["K"], f["V"], S_SIGNED, dtype)
    assert HC.bits_equal(O[0], Os) and HC.bits_equal(L[0], Ls)
    g = HC.heads_backward_once(heads, [b], 1, 1, "bhmd", S_SIGNED, dtype)
    gs = BC.backward_once(single, b["Q"], b["K"], b["V"], b["O"], b["GO"], b["LSE"], S_SIGNED, dtype)
    for k in HC.OUTPUTS:
        assert HC.bits_equal(g[k][0], gs[k]), k
    # the two plans hold the same state: one slice prepared, the same bytes
    assert heads.attention_stats() == single.attention_stats()
    assert heads.attention_backward_stats() == single.attention_backward_stats()
    assert single.attention_heads_prepared(D, Dv, 1) and heads.attention_prepared(D, Dv)
    assert single.attention_backward_heads_prepared(D, Dv, 1) and heads.attention_backward_prepared(D, Dv)
    if single.attention_stats()["partials"]:
        assert not heads.attention_heads_prepared(D, Dv, 2)
