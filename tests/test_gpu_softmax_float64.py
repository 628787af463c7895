"""GPU: values of the row softmax over the plan's pattern (bsmr_softmax, bsmr_softmax_backward)
against the float64 reference; data, bounds and their derivation: tests/softmax_cases.py.

Patterns: staircase (every row length 0 .. 271: every packed class, every fill of a run, wave
rows), hub (one block row of 2048), zipf_shuffled, empty, and long (rows of wave_max, wave_max + 1,
block_pass, block_pass + 1 and 2 block_pass + 37, the sizes taken from the library). Scales 1,
0.125 and 1 / sqrt(64).

Forward: one-hot data bit for bit (hot place (7 i) mod len; on `long` also first, last and both
sides of every pass boundary); shift invariance bit for bit on the 1/8 grid; window data on `long`
(within the bound of 1/64 inside, exactly 0 outside); signed narrow and wide data within
forward_bound, row sums within theirs; W starts as a bit pattern and every entry is written,
nothing behind the last; in place == out of place, two launches, a lazily built and a prepared
plan, and two streams at once are all bitwise equal.

Backward: grid data bit for bit (exact in any summation order), signed data within backward_bound,
in place == out of place.

The worst ratios are printed ("RATIO softmax/...") for DESIGN.md section 12.
"""
import functools

import numpy as np
import pytest

from gpu_util import torch_cuda
from softmax_cases import (PATTERNS, SCALES, backward_grid, backward_once, backward_ratio, backward_ref,
                           backward_signed, check_exact, check_forward, check_window, dev, expected_stats, filled,
                           grid_scores, long_hot_places, make_plan, one_hot, pattern, row_shifts, signed_scores,
                           softmax_once, window)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _plan(name):
    return make_plan(pattern(name))


@pytest.mark.parametrize("name", PATTERNS)
def test_one_hot_is_bit_exact(name):
    pat, plan = pattern(name), _plan(name)
    for where in ["mod7"] + (long_hot_places() if name == "long" else []):
        P, want = one_hot(pat, where)
        for scale in SCALES:
            check_exact(softmax_once(plan, P, scale), want, pat, f"{name} hot {where} scale {scale}")
    assert plan.softmax_stats() == expected_stats(pat)


@pytest.mark.parametrize("name", PATTERNS)
def test_shift_invariance_is_bitwise(name):
    pat, plan = pattern(name), _plan(name)
    P = grid_scores(pat, 3)
    for scale in SCALES:
        W = softmax_once(plan, P, scale)
        check_forward(W, pat, P, scale, f"{name} grid scale {scale}", "grid")
        check_exact(softmax_once(plan, P + row_shifts(pat), scale), W, pat, f"{name} shifted scale {scale}")


@pytest.mark.parametrize("where", ["tail", "boundary"])
def test_window_data_on_the_long_rows(where):
    pat, plan = pattern("long"), _plan("long")
    P, inside = window(pat, where)
    for scale in SCALES:
        check_window(softmax_once(plan, P, scale), pat, inside, f"long window {where} scale {scale}")


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("name", PATTERNS)
def test_signed_data_within_the_bound(name, kind):
    pat, plan = pattern(name), _plan(name)
    P = signed_scores(pat, kind, 11)
    for scale in SCALES:
        check_forward(softmax_once(plan, P, scale), pat, P, scale, f"{name} {kind} scale {scale}", kind)


@pytest.mark.parametrize("name", PATTERNS)
def test_in_place_repeat_and_prepared_are_bitwise_equal(name):
    torch = torch_cuda()
    pat, plan = pattern(name), _plan(name)
    P = signed_scores(pat, "wide", 13)
    W = softmax_once(plan, P, 0.125)
    assert np.array_equal(W.view(np.uint32), softmax_once(plan, P, 0.125).view(np.uint32)), "two launches differ"
    d = dev(P)
    plan.softmax(d.data_ptr(), d.data_ptr(), 0.125, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check_exact(d.cpu().numpy()[:len(P)], W, pat, f"{name} in place")
    fresh = make_plan(pat)
    assert not fresh.softmax_prepared() and fresh.softmax_stats()["items"] == 0
    fresh.prepare_softmax()
    fresh.prepare_softmax()  # idempotent
    assert fresh.softmax_prepared() and fresh.softmax_stats() == expected_stats(pat)
    check_exact(softmax_once(fresh, P, 0.125), W, pat, f"{name} prepared plan")
    lazy = make_plan(pat)
    check_exact(softmax_once(lazy, P, 0.125), W, pat, f"{name} lazily built plan")
    assert lazy.softmax_prepared()


@pytest.mark.parametrize("name", ["long", "zipf_shuffled"])
def test_two_streams_at_once_equal_the_serial_results(name):
    torch = torch_cuda()
    pat, plan = pattern(name), _plan(name)
    Pa, Pb = signed_scores(pat, "wide", 17), signed_scores(pat, "narrow", 19)
    serial = softmax_once(plan, Pa, 1.0), softmax_once(plan, Pb, 0.125)
    da, db = dev(Pa), dev(Pb)
    (_, wa), (_, wb) = filled(len(Pa)), filled(len(Pb))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ready = torch.cuda.Event()
    ready.record()
    s1.wait_event(ready)
    s2.wait_event(ready)
    plan.softmax(da.data_ptr(), wa.data_ptr(), 1.0, stream=s1.cuda_stream)
    plan.softmax(db.data_ptr(), wb.data_ptr(), 0.125, stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    check_exact(wa.cpu().numpy()[:len(Pa)], serial[0], pat, f"{name} stream 1")
    check_exact(wb.cpu().numpy()[:len(Pb)], serial[1], pat, f"{name} stream 2")


@pytest.mark.parametrize("name", PATTERNS)
def test_backward_grid_data_is_bit_exact(name):
    torch = torch_cuda()
    pat, plan = pattern(name), _plan(name)
    W, G = backward_grid(pat, 21)
    for scale in (1.0, 0.125, 2.0):
        want = backward_ref(pat, W, G, scale)["dP"].astype(np.float32)
        check_exact(backward_once(plan, W, G, scale), want, pat, f"{name} backward grid scale {scale}")
    dW, dG = dev(W), dev(G)
    plan.softmax_backward(dW.data_ptr(), dG.data_ptr(), dG.data_ptr(), 2.0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check_exact(dG.cpu().numpy()[:len(W)], want, pat, f"{name} backward in place")
    assert np.array_equal(dW.cpu().numpy()[:len(W)], W)


@pytest.mark.parametrize("name", PATTERNS)
def test_backward_signed_data_within_the_bound(name):
    pat, plan = pattern(name), _plan(name)
    for scale in SCALES:
        W, G = backward_signed(pat, scale, 23)
        ratio = backward_ratio(backward_once(plan, W, G, scale), backward_ref(pat, W, G, scale))
        print(f"RATIO softmax/backward {ratio:.4f} {name} scale {scale}")
        assert ratio <= 1.0, f"{name} scale {scale}: worst |dP - ref| / bound = {ratio:.3f}"
