"""CPU: the softmax checker checks itself (tests/softmax_cases.py; no GPU).

The numpy-fp32 emulation of the documented summation order (softmax_emulate, over the library's own
host item list) must pass every check the GPU tests apply: one-hot data bit for bit at every scale
and hot place, shift invariance bit for bit, window data, signed data within forward_bound with row
sums within theirs, and the backward on grid data bit for bit and on signed data within
backward_bound.

Five mutations of the emulation, each a subtly wrong kernel, must each fail a check on rows of
n <= 2048 (staircase and hub): every mutation that changes a term's index fails bit equality on
one-hot data, the bf16 rounding fails the signed bound, and the dropped wave partial also fails the
window check on the `long` rows. Dropping one term of a narrow row of 2048 must stand well above the
bound (it is invisible in a row of block_pass + 1, which is why the long rows have window data).
"""
import numpy as np
import pytest

from softmax_cases import (INDEX_MUTATIONS, MUTATIONS, PATTERNS, SCALES, SMALLEST, backward_emulate, backward_grid,
                           backward_ratio, backward_ref, backward_signed, check_exact, check_forward, check_window,
                           forward_ratio, grid_scores, limits, long_hot_places, one_hot, pattern, row_lengths,
                           row_shifts, signed_scores, softmax_emulate, softmax_ref, window)

SHORT = ["staircase", "hub"]  # rows of n <= 2048


def _fails(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", PATTERNS + SMALLEST)
def test_emulation_is_exact_on_one_hot_data(name):
    pat = pattern(name)
    places = ["mod7"] + (long_hot_places() if name == "long" else ["last", 0])
    for where in places:
        P, want = one_hot(pat, where)
        for scale in (SCALES if where == "mod7" else SCALES[1:2]):
            check_exact(softmax_emulate(pat, P, scale), want, pat, f"{name} hot {where} scale {scale}")


@pytest.mark.parametrize("name", PATTERNS)
def test_emulation_is_shift_invariant_bitwise(name):
    pat = pattern(name)
    P = grid_scores(pat, 3)
    for scale in SCALES:
        W = softmax_emulate(pat, P, scale)
        check_exact(softmax_emulate(pat, P + row_shifts(pat), scale), W, pat, f"{name} shifted scale {scale}")


def test_emulation_on_window_data():
    pat = pattern("long")
    for where in ("tail", "boundary"):
        P, inside = window(pat, where)
        for scale in SCALES:
            check_window(softmax_emulate(pat, P, scale), pat, inside, f"long window {where} scale {scale}")


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("name", PATTERNS)
def test_emulation_within_the_signed_bound(name, kind):
    pat = pattern(name)
    P = signed_scores(pat, kind, 11)
    worst = max(check_forward(softmax_emulate(pat, P, s), pat, P, s, f"{name} {kind} scale {s}", "emulated")
                for s in SCALES)
    assert worst < 0.5  # the emulation sits well inside (0.26 at worst when this was written)


@pytest.mark.parametrize("name", PATTERNS)
def test_backward_emulation(name):
    pat = pattern(name)
    W, G = backward_grid(pat, 21)
    for scale in (1.0, 0.125):
        ref = backward_ref(pat, W, G, scale)
        check_exact(backward_emulate(pat, W, G, scale), ref["dP"].astype(np.float32), pat, f"{name} grid {scale}")
        assert (ref["dP"].astype(np.float32).astype(np.float64) == ref["dP"]).all()  # exact in fp32
    for scale in SCALES:
        W, G = backward_signed(pat, scale, 23)
        ratio = backward_ratio(backward_emulate(pat, W, G, scale), backward_ref(pat, W, G, scale))
        assert ratio <= 1.0, (name, scale, ratio)


@pytest.mark.parametrize("mutation", INDEX_MUTATIONS)
def test_index_mutations_fail_bit_equality_on_one_hot_data(mutation):
    failed = []
    for name in SHORT:
        pat = pattern(name)
        for where in ("mod7", "last", 0):
            P, want = one_hot(pat, where)
            with np.errstate(all="ignore"):
                W = softmax_emulate(pat, P, 0.125, mutation)
            if _fails(check_exact, W, want, pat, "mutated"):
                failed.append((name, where))
    assert failed, f"{mutation}: no one-hot check on rows of n <= 2048 fails"
    if mutation == "drop_last_partial":
        assert all(n == "hub" for n, _ in failed)  # (staircase has no block row)


def test_every_mutation_fails_a_check_on_short_rows():
    for mutation in MUTATIONS:
        bad = 0
        for name in SHORT:
            pat = pattern(name)
            P = signed_scores(pat, "narrow", 11)
            with np.errstate(all="ignore"):
                W = softmax_emulate(pat, P, 1.0, mutation)
            bad += forward_ratio(W, softmax_ref(pat, P, 1.0)) > 1.0
            P, want = one_hot(pat, "last")
            with np.errstate(all="ignore"):
                bad += _fails(check_exact, softmax_emulate(pat, P, 1.0, mutation), want, pat, "mutated")
        assert bad, f"{mutation}: every check passes"


def test_bf16_rounding_fails_the_signed_bound():
    for name in SHORT:
        pat = pattern(name)
        P = signed_scores(pat, "narrow", 11)
        assert forward_ratio(softmax_emulate(pat, P, 1.0, "round_bf16"), softmax_ref(pat, P, 1.0)) > 100


def test_one_dropped_term_of_a_narrow_row_of_2048_stands_above_the_bound():
    pat = pattern("hub")
    hub = row_lengths(pat) == 2048
    assert hub.sum() == 1
    P = signed_scores(pat, "narrow", 11)
    ref = softmax_ref(pat, P, 1.0)
    mask = np.repeat(hub, row_lengths(pat))
    ok = forward_ratio(softmax_emulate(pat, P, 1.0), ref, mask)
    dropped = forward_ratio(softmax_emulate(pat, P, 1.0, "drop_last_term"), ref, mask)
    print(f"hub row: emulation {ok:.3f} of the bound, one term dropped {dropped:.1f}")
    assert ok <= 1.0 and dropped > 5.0


def test_dropped_partial_fails_on_the_long_rows_with_window_data():
    pat = pattern("long")
    w = limits()["wave_max"]
    for where in ("tail", "boundary"):
        P, inside = window(pat, where)
        W = softmax_emulate(pat, P, 0.125, "drop_last_partial")
        assert _fails(check_window, W, pat, inside, "mutated"), where
        # exactly the block rows are wrong
        good = softmax_emulate(pat, P, 0.125)
        wrong = np.unique(np.repeat(np.arange(pat[0]), row_lengths(pat))[W != good])
        assert len(wrong) and (row_lengths(pat)[wrong] > w).all()
