"""GPU: edges of the fused sparse attention backward (bsmr_attention_backward).

* every smallest legal plan (tests/small_patterns.py; bsmr_plan_create needs two entries, so 1 x 2
  and 2 x 1 stand for 1 x 1 and the plan without entries): both exact sets bit for bit, signed data
  inside the bound, stats as the list lengths give them; empty rows and empty columns give exact
  zeros;
* guard zones: every launch goes through attention_bwd_cases.backward_once, whose three outputs are
  pre-filled and padded: every element of a requested output is written, no pad word changes;
* NaN / +inf containment: one poisoned row of Q, K, V, GO, O and LSE in turn; only the destinations
  the header names may change, every other element equals the clean run bit for bit, and the
  destinations a NaN must reach are NaN;
* rows with LSE = -inf give GQ = 0 and add nothing to GK and GV;
* BSMR_ERR_INVALID for a null plan or pointer, three null outputs, a misaligned pointer and a bad
  scale, BSMR_ERR_UNSUPPORTED for a dtype, D or Dv off the rules or rows over the byte cap: the
  pre-filled outputs stay untouched and nothing is built;
* graph capture: unprepared, BSMR_ERR_NOT_PREPARED and the capture stays usable; after
  prepare_attention_backward the first launch of a fresh plan is captured and replayed twice with
  equal bits, equal to the direct launch.
"""
import numpy as np
import pytest

import attention_bwd_cases as BC
import bsmr
from bsmr import BF16, F16, F32
from gpu_util import torch_cuda
from softmax_cases import FILL_BITS, SMALLEST, filled

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 6


def _bits_equal(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


@pytest.mark.parametrize("name", SMALLEST)
def test_smallest_plans(name):
    pat = BC.pattern(name)
    plan = BC.make_plan(pat)
    assert plan.attention_backward_stats() == BC.expected_stats(pat, built=False)
    top = (0, 0)
    for dtype, D, Dv in ((F32, 16, 16), (F32, 32, 48), (BF16, 32, 64)):
        what = f"{name} {BC.DTYPE_NAME[dtype]} {D}x{Dv}"
        Q, K, V, O, GO, LSE, winner = BC.selector_inputs(pat, D, Dv, "random", 0.125, dtype)
        got = BC.backward_once(plan, Q, K, V, O, GO, LSE, 0.125, dtype)
        for k, w in zip(BC.OUTPUTS, BC.selector_expected(pat, GO, winner, D, Dv)):
            BC.check_exact(got[k], w, f"{k} selector {what}")
        inputs = BC.flat_inputs(pat, D, Dv, dtype)
        BC.check_exact_all(BC.backward_once(plan, *inputs, 0.125, dtype), BC.backward_ref(pat, *inputs, 0.125, dtype),
                           f"flat {what}")
        Q, K, V, O, GO, LSE, opscale, _ = BC.signed_inputs(pat, D, Dv, "wide", 0.25, dtype)
        BC.check_bound(BC.backward_once(plan, Q, K, V, O, GO, LSE, 0.25, dtype),
                       BC.backward_ref(pat, Q, K, V, O, GO, LSE, 0.25, dtype), what, opscale)
        top = (max(top[0], D), max(top[1], D + Dv))
    want = BC.expected_stats(pat, 1, 0)
    want["row_scratch_bytes"] = 4 * want["row_partials"] * top[0]
    want["col_scratch_bytes"] = 4 * want["col_partials"] * top[1]
    assert plan.attention_backward_stats() == want


@pytest.mark.parametrize("name", ["empty", "empty_T", "long4", "hub_T"])
def test_stats_and_empty_destinations(name):
    pat = BC.pattern(name)
    plan = BC.make_plan(pat)
    plan.prepare_attention_backward(64, 32)
    assert plan.attention_backward_stats() == BC.expected_stats(pat, 64, 32)
    plan.prepare_attention_backward(32, 32)  # a smaller shape keeps the scratch
    assert plan.attention_backward_stats() == BC.expected_stats(pat, 64, 32)
    Q, K, V, O, GO, LSE, _, _ = BC.signed_inputs(pat, 64, 32, "narrow", 1.0)
    got = BC.backward_once(plan, Q, K, V, O, GO, LSE, 1.0)
    rows0, cols0 = BC.AC.row_lengths(pat) == 0, BC.col_lengths(pat) == 0
    assert (got["GQ"][rows0].view(np.uint32) == 0).all(), "an empty row of GQ is not +0"
    assert (got["GK"][cols0].view(np.uint32) == 0).all() and (got["GV"][cols0].view(np.uint32) == 0).all()
    assert all(np.isfinite(got[k]).all() for k in BC.OUTPUTS)


@pytest.mark.parametrize("dtype,D,Dv", [(F32, 32, 48), (F16, 64, 64)])
@pytest.mark.parametrize("what", ["Q", "K", "V", "GO", "O", "LSE"])
@pytest.mark.parametrize("name", ["staircase", "zipf_shuffled"])
def test_nan_and_inf_stay_in_their_destinations(name, what, dtype, D, Dv):
    pat = BC.pattern(name)
    M, N, rp, ci = pat
    plan = BC.make_plan(pat)
    Q, K, V, O, GO, LSE, _, _ = BC.signed_inputs(pat, D, Dv, "wide", 0.25, dtype)
    args = dict(Q=Q, K=K, V=V, O=O, GO=GO, LSE=LSE)
    clean = BC.backward_once(plan, Q, K, V, O, GO, LSE, 0.25, dtype)
    rows, cols = BC.AC.entry_rows(pat), np.asarray(ci, np.int64)
    if what in ("K", "V"):
        refs = np.bincount(ci, minlength=N).astype(np.float64)
        refs[(refs == 0) | (refs >= M)] = np.inf
        target = int(np.abs(refs - M / 3).argmin())  # a column that about a third of the rows reference
        hitQ = np.zeros(M, bool)
        hitQ[rows[cols == target]] = True
        hitKV = np.zeros(N, bool)
        hitKV[target] = True
    else:
        lens = BC.AC.row_lengths(pat)
        target = int(np.abs(lens - lens.max() / 3).argmin()) if name == "zipf_shuffled" else int(lens.argmax()) // 3
        hitQ = np.zeros(M, bool)
        hitQ[target] = True
        hitKV = np.zeros(N, bool)
        hitKV[cols[rows == target]] = True
    assert hitQ.any() and not hitQ.all() and hitKV.any() and not hitKV.all()
    for poison in (np.nan, np.inf):
        X = args[what].copy()
        X[target] = poison
        a = dict(args)
        a[what] = X
        got = BC.backward_once(plan, a["Q"], a["K"], a["V"], a["O"], a["GO"], a["LSE"], 0.25, dtype)
        tag = f"{what} {poison}"
        assert _bits_equal(got["GQ"][~hitQ], clean["GQ"][~hitQ]), f"{tag}: a GQ row outside the named ones changed"
        assert _bits_equal(got["GK"][~hitKV], clean["GK"][~hitKV]), f"{tag}: a GK row outside the named ones changed"
        assert _bits_equal(got["GV"][~hitKV], clean["GV"][~hitKV]), f"{tag}: a GV row outside the named ones changed"
        if np.isnan(poison):
            # what the definition must turn into NaN: w (Q, K, LSE), g (GO, V), delta (GO, O) enter dp; w and GO enter GV
            assert np.isnan(got["GQ"][hitQ]).all(), f"{tag}: a named GQ row is not NaN in every column"
            assert np.isnan(got["GK"][hitKV]).all(), f"{tag}: a named GK row is not NaN in every column"
            if what in ("Q", "K", "LSE", "GO"):
                assert np.isnan(got["GV"][hitKV]).all(), f"{tag}: a named GV row is not NaN in every column"
            else:
                assert _bits_equal(got["GV"], clean["GV"]), f"{tag}: {what} does not enter GV"
        else:
            changed = (got["GQ"].view(np.uint32) != clean["GQ"].view(np.uint32)).any(axis=1)
            assert changed[hitQ].all(), f"{tag}: a named GQ row did not change"


def test_minus_inf_lse_rows_give_zeros_and_add_nothing():
    pat = BC.pattern("staircase")
    M = pat[0]
    plan = BC.make_plan(pat)
    D, Dv = 32, 48
    Q, K, V, O, GO, LSE, opscale, _ = BC.signed_inputs(pat, D, Dv, "wide", 0.25)
    masked = np.arange(M) % 3 == 1
    L2 = LSE.copy()
    L2[masked] = -np.inf
    got = BC.backward_once(plan, Q, K, V, O, GO, L2, 0.25)
    assert (got["GQ"][masked].view(np.uint32) == 0).all(), "a row with LSE = -inf has a GQ other than +0"
    # the reference gives those rows' entries weight 0: they add nothing to GK and GV
    ref = BC.backward_ref(pat, Q, K, V, O, GO, L2, 0.25)
    assert (ref["w"][masked[ref["rows"]]] == 0).all()
    BC.check_bound(got, ref, "LSE = -inf rows", opscale)


def test_errors_leave_the_outputs_untouched():
    torch = torch_cuda()
    pat = BC.pattern("long4")
    plan = BC.make_plan(pat)
    M, N = pat[0], pat[1]
    s = torch.cuda.current_stream().cuda_stream
    z = lambda n: torch.zeros(n, dtype=torch.float32, device="cuda")  # noqa: E731
    dQ, dK, dV, dO, dGO, dL = z(M * 256), z(N * 256), z(N * 256), z(M * 256), z(M * 256), z(M)
    bufs = [filled(M * 256), filled(N * 256), filled(N * 256)]
    q, k, v, o, go, l = (t.data_ptr() for t in (dQ, dK, dV, dO, dGO, dL))
    gq, gk, gv = (b[1].data_ptr() for b in bufs)

    def status(*a, **kw):
        with pytest.raises(bsmr.BsmrError) as ei:
            plan.attention_backward(*a, **kw)
        return ei.value.status, str(ei.value)

    for scale in (0.0, -1.0, float("nan"), float("inf"), 3e38):
        st, msg = status(q, k, v, o, go, l, 64, 64, gq, gk, gv, scale, stream=s)
        assert st == INVALID and "scale" in msg, (scale, msg)
    for i in range(6):
        a = [q, k, v, o, go, l]
        a[i] = 0
        assert status(*a, 64, 64, gq, gk, gv, 1.0, stream=s)[0] == INVALID, i
    st, msg = status(q, k, v, o, go, l, 64, 64, 0, 0, 0, 1.0, stream=s)
    assert st == INVALID and "all null" in msg
    for i in range(5):
        a = [q, k, v, o, go, l]
        a[i] += 4
        assert status(*a, 64, 64, gq, gk, gv, 1.0, stream=s)[0] == INVALID, i
    assert status(q, k, v, o, go, l + 2, 64, 64, gq, gk, gv, 1.0, stream=s)[0] == INVALID
    for outs in ((gq + 8, gk, gv), (gq, gk + 4, gv), (gq, gk, gv + 8), (0, gk + 8, 0)):
        assert status(q, k, v, o, go, l, 64, 64, *outs, 1.0, stream=s)[0] == INVALID
    assert bsmr.lib().bsmr_attention_backward(None, q, k, v, o, go, l, 64, 64, F32, 1.0, gq, gk, gv, None) == INVALID
    cap = BC.limits()["max_row_bytes"]
    bad_dims = [(F32, 0, 64), (F32, 64, 0), (F32, 24, 64), (F32, 64, 40), (F32, cap // 4 + 16, 64),
                (F32, 64, cap // 4 + 16), (F16, 48, 64), (BF16, 64, 40), (F16, 16, 64), (BF16, cap // 2 + 32, 64),
                (F16, 64, cap // 2 + 32), (3, 64, 64)]
    for dtype, D, Dv in bad_dims:
        st, msg = status(q, k, v, o, go, l, D, Dv, gq, gk, gv, 1.0, stream=s, dtype=dtype)
        assert st == UNSUPPORTED, (dtype, D, Dv, msg)
    torch.cuda.synchronize()
    for name, (buf, _) in zip(BC.OUTPUTS, bufs):
        assert (buf.cpu().numpy().view(np.uint32) == FILL_BITS).all(), f"a refused call wrote {name}"
    assert not plan.attention_backward_prepared(64, 64)
    assert plan.attention_backward_stats() == BC.expected_stats(pat, built=False)
    with pytest.raises(bsmr.BsmrError):
        plan.prepare_attention_backward(24, 64)
    assert not plan.attention_backward_prepared(24, 64)
    # the largest legal rows pass
    plan.attention_backward(q, k, v, o, go, l, cap // 4, cap // 4, gq, gk, gv, 1.0, stream=s)
    torch.cuda.synchronize()


def _capture(torch, fn):
    """fn(stream) recorded into a graph on a side stream (a plain chain of nodes)."""
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(side.cuda_stream)
    return g


def test_capture_needs_a_prepared_plan():
    torch = torch_cuda()
    pat = BC.pattern("long4_T")
    M, N = pat[0], pat[1]
    D, Dv, scale = 32, 48, 0.25
    inputs = BC.signed_inputs(pat, D, Dv, "wide", scale)[:6]
    dev = BC.device_inputs(*inputs)
    plan = BC.make_plan(pat)
    shapes = ((M, D), (N, D), (N, Dv))
    bufs = [filled(r * c) for r, c in shapes]
    marker = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    caught = []

    def launch(s):
        plan.attention_backward(*(t.data_ptr() for t in dev), D, Dv, *(b[1].data_ptr() for b in bufs), scale, stream=s)

    def refused(s):
        marker.zero_()
        with pytest.raises(bsmr.BsmrError) as ei:
            launch(s)
        caught.append(ei.value)

    g = _capture(torch, refused)  # ends normally: the refused launch did not invalidate the capture
    assert caught[0].status == bsmr.NOT_PREPARED
    assert "bsmr_attention_backward: stream is capturing" in str(caught[0])
    assert "bsmr_plan_prepare_attention_backward first" in str(caught[0])
    marker.fill_(1)
    g.replay()
    torch.cuda.synchronize()
    assert float(marker.cpu()[0]) == 0, "the capture did not stay usable"
    for buf, _ in bufs:
        assert (buf.cpu().numpy().view(np.uint32) == FILL_BITS).all()
    assert not plan.attention_backward_prepared(D, Dv)

    plan.prepare_attention_backward(D, Dv)
    assert plan.attention_backward_prepared(D, Dv) and plan.attention_backward_prepared(D, 16)
    assert not plan.attention_backward_prepared(D, 64), "the scratch of Dv = 48 does not hold the partials of Dv = 64"
    g = _capture(torch, launch)  # the plan's first launch
    direct = BC.backward_once(BC.make_plan(pat), *inputs, scale, dev=dev)
    for replay in (1, 2):
        for _, view in bufs:
            view.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k, (buf, _), (r, c) in zip(BC.OUTPUTS, bufs, shapes):
            h = buf.cpu().numpy()
            assert _bits_equal(h[:r * c].reshape(r, c), direct[k]), f"replay {replay}: {k} differs from the direct launch"
            assert (h[r * c:].view(np.uint32) == FILL_BITS).all()
