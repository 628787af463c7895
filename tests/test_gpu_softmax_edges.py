"""GPU: the edges of the row softmax over the plan's pattern (reference, data and bounds:
tests/softmax_cases.py).

* the smallest legal plans (tests/small_patterns.py), forward (one-hot, bit for bit) and backward
  (grid data, bit for bit), with the stats;
* guard zones: P, W and G inside larger buffers (4096 elements before and after: NaN around the
  inputs, a bit pattern around the outputs), once 16-byte aligned and once one element off (every
  row then takes the 4-byte loads), on `long` and `staircase`: forward exact on one-hot data,
  backward exact on grid data, the guards and the inputs unchanged. The guards are passive:
  nothing here reads or writes out of bounds on purpose;
* NaN and inf containment: one NaN and one +inf in P: exactly those two rows are NaN and every other
  row stays within the bound; one -inf: weight exactly 0 and the row's others within the bound of
  the reference without it; a row all -inf: zeros forward and backward;
* invalid scales and null pointers from every entry point: BSMR_ERR_INVALID, outputs untouched;
* graph capture: unprepared, BSMR_ERR_NOT_PREPARED and the capture stays usable; after
  prepare_softmax the first launch of a fresh plan is captured and replayed on a P changed in
  place; softmax_prepared is 0 before and 1 after, and recolumn leaves it 1.
"""
import numpy as np
import pytest

import bsmr
from gpu_util import torch_cuda
from softmax_cases import (FILL_BITS, PATTERNS, backward_grid, backward_once, backward_ref, check_exact, dev,
                           entry_rows, expected_stats, filled, forward_ratio, make_plan, one_hot, pattern,
                           row_lengths, signed_scores, softmax_once, softmax_ref, SMALLEST)

pytestmark = pytest.mark.gpu

GUARD = 4096
INVALID = 1


def _cur(torch):
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", SMALLEST)
def test_smallest_plans(name):
    pat = pattern(name)
    plan = make_plan(pat)
    for where in ("mod7", "last"):
        P, want = one_hot(pat, where)
        check_exact(softmax_once(plan, P, 0.125), want, pat, f"{name} hot {where}")
    W, G = backward_grid(pat, 31)
    check_exact(backward_once(plan, W, G, 0.5), backward_ref(pat, W, G, 0.5)["dP"].astype(np.float32), pat,
                f"{name} backward")
    assert plan.softmax_stats() == expected_stats(pat)


def _guarded(torch, x, off, nan):
    """x inside a buffer with GUARD (+ off) elements around it: NaN (inputs) or FILL_BITS (outputs)."""
    n = len(x)
    buf = torch.full((n + 2 * GUARD + off,), FILL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    if nan:
        buf.fill_(float("nan"))
    mid = buf[GUARD + off:GUARD + off + n]
    if nan:
        mid.copy_(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())
    return buf, mid


def _bits(t):
    return t.view(torch_cuda().int32)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off_by_one"])
@pytest.mark.parametrize("name", ["long", "staircase"])
def test_guard_zones(name, off):
    torch = torch_cuda()
    pat, plan = pattern(name), make_plan(pattern(name))
    nnz = len(pat[3])
    P, want = one_hot(pat, "mod7")
    bufP, dP = _guarded(torch, P, off, True)
    bufW, dW = _guarded(torch, np.zeros(nnz), off, False)
    assert dP.data_ptr() % 16 == 4 * off and dW.data_ptr() % 16 == 4 * off
    keepP = _bits(bufP).clone()
    plan.softmax(dP.data_ptr(), dW.data_ptr(), 0.125, stream=_cur(torch))
    torch.cuda.synchronize()
    host = bufW.cpu().numpy()
    assert (host[:GUARD + off].view(np.uint32) == FILL_BITS).all(), "a store before W[0]"
    assert (host[GUARD + off + nnz:].view(np.uint32) == FILL_BITS).all(), "a store past W"
    check_exact(host[GUARD + off:GUARD + off + nnz], want, pat, f"{name} guarded forward")
    assert torch.equal(_bits(bufP), keepP)

    W, G = backward_grid(pat, 33)
    bufWi, dWi = _guarded(torch, W, off, True)
    bufG, dG = _guarded(torch, G, off, True)
    bufO, dO = _guarded(torch, np.zeros(nnz), off, False)
    keepW, keepG = _bits(bufWi).clone(), _bits(bufG).clone()
    plan.softmax_backward(dWi.data_ptr(), dG.data_ptr(), dO.data_ptr(), 0.25, stream=_cur(torch))
    torch.cuda.synchronize()
    host = bufO.cpu().numpy()
    assert (host[:GUARD + off].view(np.uint32) == FILL_BITS).all(), "a store before dP[0]"
    assert (host[GUARD + off + nnz:].view(np.uint32) == FILL_BITS).all(), "a store past dP"
    check_exact(host[GUARD + off:GUARD + off + nnz], backward_ref(pat, W, G, 0.25)["dP"].astype(np.float32), pat,
                f"{name} guarded backward")
    assert torch.equal(_bits(bufWi), keepW) and torch.equal(_bits(bufG), keepG)


def _row_entry(pat, want_len_at_least, skip=()):
    """(row, CSR position of an entry in its middle) of the longest row not in `skip`."""
    lens = row_lengths(pat).copy()
    lens[list(skip)] = 0
    r = int(lens.argmax())
    assert lens[r] >= want_len_at_least
    return r, int(pat[2][r]) + int(lens[r]) // 2


@pytest.mark.parametrize("name", PATTERNS)
def test_nan_and_inf_stay_in_their_rows(name):
    pat, plan = pattern(name), make_plan(pattern(name))
    rows = entry_rows(pat)
    P = signed_scores(pat, "wide", 41)
    r1, e1 = _row_entry(pat, 2)
    r2, e2 = _row_entry(pat, 2, skip=(r1,))
    P[e1], P[e2] = np.nan, np.inf
    W = softmax_once(plan, P, 0.125)
    hit = (rows == r1) | (rows == r2)
    assert np.isnan(W[hit]).all(), "a NaN / +inf row holds an entry that is not NaN"
    ref = softmax_ref(pat, P, 0.125)
    assert np.isnan(ref["W"][hit]).all() and np.isfinite(ref["W"][~hit]).all()
    ratio = forward_ratio(W, ref, ~hit)
    assert ratio <= 1.0, f"{name}: rows beside the NaN / +inf rows: {ratio:.3f} of the bound"

    # one -inf: weight exactly 0, the row's others as if it were not there
    P = signed_scores(pat, "wide", 43)
    P[e1] = -np.inf
    W = softmax_once(plan, P, 0.125)
    assert W[e1] == 0 and np.isfinite(W).all()
    ref = softmax_ref(pat, P, 0.125)
    assert ref["W"][e1] == 0
    ref["n"][rows == r1] -= 1  # the bound of the row without the masked entry
    assert forward_ratio(W, ref) <= 1.0

    # rows all -inf: zeros forward, zeros backward
    P = signed_scores(pat, "wide", 45)
    masked = (rows == r1) | (rows == r2)
    P[masked] = -np.inf
    W = softmax_once(plan, P, 0.125)
    assert (W[masked] == 0).all() and forward_ratio(W, softmax_ref(pat, P, 0.125)) <= 1.0
    G = signed_scores(pat, "narrow", 47)
    dP = backward_once(plan, W, G, 0.125)
    assert (dP[masked] == 0).all() and np.isfinite(dP).all()


def test_invalid_arguments_leave_the_outputs_untouched():
    torch = torch_cuda()
    pat = pattern("empty")
    plan = make_plan(pat)
    nnz = len(pat[3])
    dP, dG = dev(signed_scores(pat, "narrow", 51)), dev(signed_scores(pat, "narrow", 53))
    buf, dW = filled(nnz)
    s = _cur(torch)
    for scale in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 3e38):
        for call in (lambda: plan.softmax(dP.data_ptr(), dW.data_ptr(), scale, stream=s),
                     lambda: plan.softmax_backward(dP.data_ptr(), dG.data_ptr(), dW.data_ptr(), scale, stream=s)):
            with pytest.raises(bsmr.BsmrError) as ei:
                call()
            assert ei.value.status == INVALID and "scale" in str(ei.value), str(ei.value)
    L = bsmr.lib()
    p, w, g = dP.data_ptr(), dW.data_ptr(), dG.data_ptr()
    assert L.bsmr_softmax(None, p, 1.0, w, None) == INVALID
    assert L.bsmr_softmax(plan.h, None, 1.0, w, None) == INVALID
    assert L.bsmr_softmax(plan.h, p, 1.0, None, None) == INVALID
    assert L.bsmr_softmax_backward(None, p, g, 1.0, w, None) == INVALID
    assert L.bsmr_softmax_backward(plan.h, None, g, 1.0, w, None) == INVALID
    assert L.bsmr_softmax_backward(plan.h, p, None, 1.0, w, None) == INVALID
    assert L.bsmr_softmax_backward(plan.h, p, g, 1.0, None, None) == INVALID
    assert L.bsmr_plan_prepare_softmax(None) == INVALID
    assert L.bsmr_plan_softmax_prepared(None) == 0
    assert L.bsmr_plan_softmax_stats(None, bsmr.C.byref(bsmr.SoftmaxStats())) == INVALID
    assert L.bsmr_plan_softmax_stats(plan.h, None) == INVALID
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == FILL_BITS).all(), "a refused call wrote to its output"
    assert not plan.softmax_prepared()  # and none of them built the list


def _capture(torch, fn):
    """fn(stream) recorded into a graph on a side stream (a plain chain of nodes)."""
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(side.cuda_stream)
    return g


def test_unprepared_capture_reports_not_prepared():
    torch = torch_cuda()
    pat = pattern("empty")
    plan = make_plan(pat)
    P, want = one_hot(pat)
    dP = dev(P)
    buf, dW = filled(len(P))
    torch.cuda.synchronize()
    caught = []

    def body(s):
        dW.zero_()
        for call in (lambda: plan.softmax(dP.data_ptr(), dW.data_ptr(), 0.125, stream=s),
                     lambda: plan.softmax_backward(dP.data_ptr(), dP.data_ptr(), dW.data_ptr(), 0.125, stream=s)):
            with pytest.raises(bsmr.BsmrError) as ei:
                call()
            caught.append(ei.value)

    g = _capture(torch, body)  # ends normally: the refused launches did not invalidate the capture
    assert [c.status for c in caught] == [bsmr.NOT_PREPARED] * 2
    assert "bsmr_softmax: stream is capturing" in str(caught[0]) and "bsmr_plan_prepare_softmax first" in str(caught[0])
    assert "bsmr_softmax_backward: stream is capturing" in str(caught[1])
    g.replay()
    torch.cuda.synchronize()
    assert (dW.cpu().numpy() == 0).all()
    assert not plan.softmax_prepared()
    check_exact(softmax_once(plan, P, 0.125), want, pat, "lazy after the refused capture")
    assert plan.softmax_prepared()


@pytest.mark.parametrize("name", ["long", "zipf_shuffled"])
def test_first_launch_captured_after_prepare(name):
    torch = torch_cuda()
    pat = pattern(name)
    plan = make_plan(pat)
    assert not plan.softmax_prepared()
    plan.prepare_softmax()
    assert plan.softmax_prepared()
    P, want = one_hot(pat, "mod7")
    dP = dev(P)
    buf, dW = filled(len(P))
    torch.cuda.synchronize()
    g = _capture(torch, lambda s: plan.softmax(dP.data_ptr(), dW.data_ptr(), 0.125, stream=s))
    g.replay()
    torch.cuda.synchronize()
    check_exact(dW.cpu().numpy()[:len(P)], want, pat, f"{name} captured")
    # the graph reads the caller's P, not a captured copy
    P2, want2 = one_hot(pat, "last")
    dP.copy_(torch.from_numpy(P2).cuda())
    dW.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    check_exact(dW.cpu().numpy()[:len(P)], want2, pat, f"{name} replayed on a changed P")
    plan.recolumn(0.5)
    assert plan.softmax_prepared() and plan.softmax_stats() == expected_stats(pat)
    check_exact(softmax_once(plan, P, 0.125), want, pat, f"{name} after recolumn")
