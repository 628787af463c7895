"""GPU: edges of the fused sparse attention forward (bsmr_attention / Plan.attention).

* every smallest legal plan (tests/small_patterns.py): selector data bit for bit, signed data inside
  the bound, attention_stats as the row lengths give it;
* guard zones: every launch of this file goes through attention_cases.attention_once, whose outputs
  are pre-filled and padded: every element of O and LSE is written and no pad word changes; empty
  rows give O = 0 and LSE = -inf exactly;
* NaN / inf containment: one poisoned K row, V row or Q row; the rows the CSR names are NaN (a
  NaN) or differ (a +inf), every other row of O and LSE equals the clean run bit for bit;
* BSMR_ERR_INVALID for a null plan or pointer, a misaligned pointer and a bad scale,
  BSMR_ERR_UNSUPPORTED for a dtype, D or Dv off the rules or rows over the byte cap: the pre-filled
  outputs stay untouched and nothing is built;
* graph capture: unprepared, BSMR_ERR_NOT_PREPARED and the capture stays usable; after
  prepare_attention the first launch of a fresh plan is captured, and its replay equals the direct
  launch bit for bit; a prepared Dv does not cover a larger one on a plan with split rows;
* attention_stats equals spmm_cases.expected_stats(pattern, 1, chunk).
"""
import numpy as np
import pytest

import attention_cases as AC
import bsmr
import spmm_cases
from bsmr import BF16, F16, F32
from gpu_util import to_device, torch_cuda
from softmax_cases import FILL_BITS, SMALLEST, filled

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 6


def _expected_stats(pat):
    e = spmm_cases.expected_stats(pat, 1, AC.limits()["chunk"])
    return dict(segments=e["segments"], split_rows=e["split_dsts"], partials=e["partials"], max_row=e["max_list"],
                chunk=e["chunk"])


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


@pytest.mark.parametrize("name", SMALLEST)
def test_smallest_plans(name):
    pat = AC.pattern(name)
    plan = AC.make_plan(pat)
    assert plan.attention_stats() == dict(segments=0, split_rows=0, partials=0, max_row=0, chunk=AC.limits()["chunk"])
    for dtype, D, Dv in ((F32, 16, 16), (F32, 32, 48), (BF16, 32, 64)):
        Q, K, V, winner, pi, base = AC.selector(pat, D, Dv, "random", dtype)
        O, LSE = AC.attention_once(plan, Q, K, V, 0.125, dtype)
        wantO, wantL = AC.selector_expected(V, winner, pi, base, 0.125, dtype)
        AC.check_exact(O, wantO, f"O {name}")
        AC.check_exact(LSE, wantL, f"LSE {name}")
        Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, "wide", 0.25)
        AC.check_bound(*AC.attention_once(plan, Q, K, V, 0.25, dtype), AC.attention_ref(pat, Q, K, V, 0.25, dtype),
                       f"{name} {AC.DTYPE_NAME[dtype]} {D}x{Dv}", opscale)
    assert plan.attention_stats() == _expected_stats(pat)


@pytest.mark.parametrize("name", AC.PATTERNS)
def test_stats_and_empty_rows(name):
    pat = AC.pattern(name)
    plan = AC.make_plan(pat)
    plan.prepare_attention(64, 64)
    assert plan.attention_stats() == _expected_stats(pat)
    Q, K, V, _ = AC.signed_inputs(pat, 64, 64, "narrow", 1.0)
    O, LSE = AC.attention_once(plan, Q, K, V, 1.0)
    empty = AC.row_lengths(pat) == 0
    assert (O[empty].view(np.uint32) == 0).all(), "an empty row of O is not +0"
    assert (LSE[empty] == -np.inf).all() and np.isfinite(LSE[~empty]).all()


@pytest.mark.parametrize("dtype,D,Dv", [(F32, 32, 48), (F16, 64, 64)])
@pytest.mark.parametrize("what", ["K", "V", "Q"])
@pytest.mark.parametrize("name", ["staircase", "zipf_shuffled"])
def test_nan_and_inf_stay_in_their_rows(name, what, dtype, D, Dv):
    pat = AC.pattern(name)
    M, N, rp, ci = pat
    plan = AC.make_plan(pat)
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "wide", 0.25)
    O0, L0 = AC.attention_once(plan, Q, K, V, 0.25, dtype)
    rows = AC.entry_rows(pat)
    lens = AC.row_lengths(pat)
    if what == "Q":
        target = int(np.argmax(lens))  # the longest row: split where the pattern has split rows
        hit = np.zeros(M, bool)
        hit[target] = True
    else:
        refs = np.bincount(ci, minlength=N).astype(np.float64)
        refs[(refs == 0) | (refs >= M)] = np.inf
        target = int(np.abs(refs - M / 3).argmin())  # a column that about a third of the rows reference
        hit = np.zeros(M, bool)
        hit[rows[np.asarray(ci) == target]] = True
    assert hit.any() and not hit.all()
    for poison in (np.nan, np.inf):
        X = {"Q": Q, "K": K, "V": V}[what].copy()
        X[target, :] = poison
        args = dict(Q=Q, K=K, V=V)
        args[what] = X
        O, L = AC.attention_once(plan, args["Q"], args["K"], args["V"], 0.25, dtype)
        assert _same_bits(O[~hit], O0[~hit]), f"{what} {poison}: a row that does not reference the poison changed"
        assert _same_bits(L[~hit], L0[~hit]), f"{what} {poison}: an LSE outside the poisoned rows changed"
        changed = (O.view(np.uint32) != O0.view(np.uint32)).any(axis=1)
        assert changed[hit].all(), f"{what} {poison}: a row that references the poison did not change"
        if np.isnan(poison):
            assert np.isnan(O[hit]).all(), f"{what} NaN: a referencing row is not NaN in every column"
            if what != "V":
                assert np.isnan(L[hit]).all()
        if what == "V":
            assert _same_bits(L, L0), "V does not enter LSE"


def test_all_minus_inf_rows_give_zeros():
    pat = AC.pattern("staircase")
    plan = AC.make_plan(pat)
    D = Dv = 32
    M = pat[0]
    # Q = 1 in column 0, K[:, 0] = -inf for every column: every score is -inf
    Q = np.zeros((M, D), np.float32)
    Q[:, 0] = 1.0
    K = np.zeros((pat[1], D), np.float32)
    K[:, 0] = -np.inf
    V = AC.signed_data(pat[1] * Dv, 3).reshape(-1, Dv)
    O, LSE = AC.attention_once(plan, Q, K, V, 0.5)
    assert (O == 0).all() and (LSE == -np.inf).all()


def test_errors_leave_the_outputs_untouched():
    torch = torch_cuda()
    pat = AC.pattern("long4")
    plan = AC.make_plan(pat)
    M, N = pat[0], pat[1]
    s = torch.cuda.current_stream().cuda_stream
    z = lambda n: torch.zeros(n, dtype=torch.float32, device="cuda")  # noqa: E731
    dQ, dK, dV = z(M * 256), z(N * 256), z(N * 256)
    bufO, dO = filled(M * 256)
    bufL, dL = filled(M)
    q, k, v, o, l = (t.data_ptr() for t in (dQ, dK, dV, dO, dL))

    def status(*a, **kw):
        with pytest.raises(bsmr.BsmrError) as ei:
            plan.attention(*a, **kw)
        return ei.value.status, str(ei.value)

    for scale in (0.0, -1.0, float("nan"), float("inf"), 3e38):
        st, msg = status(q, k, v, 64, 64, o, l, scale, stream=s)
        assert st == INVALID and "scale" in msg, (scale, msg)
    for args in ((0, k, v), (q, 0, v), (q, k, 0)):
        assert status(*args, 64, 64, o, l, 1.0, stream=s)[0] == INVALID
    assert status(q, k, v, 64, 64, 0, l, 1.0, stream=s)[0] == INVALID
    assert status(q + 4, k, v, 64, 64, o, l, 1.0, stream=s)[0] == INVALID
    assert status(q, k, v, 64, 64, o + 8, l, 1.0, stream=s)[0] == INVALID
    assert bsmr.lib().bsmr_attention(None, q, k, v, 64, 64, F32, 1.0, o, l, None) == INVALID
    cap = AC.limits()["max_row_bytes"]
    bad_dims = [(F32, 0, 64), (F32, 64, 0), (F32, 24, 64), (F32, 64, 40), (F32, cap // 4 + 16, 64),
                (F32, 64, cap // 4 + 16), (F16, 48, 64), (BF16, 64, 40), (F16, 16, 64), (BF16, cap // 2 + 32, 64),
                (F16, 64, cap // 2 + 32), (3, 64, 64)]
    for dtype, D, Dv in bad_dims:
        st, msg = status(q, k, v, D, Dv, o, l, 1.0, stream=s, dtype=dtype)
        assert st == UNSUPPORTED, (dtype, D, Dv, msg)
    torch.cuda.synchronize()
    assert (bufO.cpu().numpy().view(np.uint32) == FILL_BITS).all(), "a refused call wrote O"
    assert (bufL.cpu().numpy().view(np.uint32) == FILL_BITS).all(), "a refused call wrote LSE"
    assert not plan.attention_prepared(64, 64) and plan.attention_stats()["segments"] == 0
    with pytest.raises(bsmr.BsmrError):
        plan.prepare_attention(24, 64)
    assert not plan.attention_prepared(24, 64)
    # the largest legal rows pass
    plan.attention(q, k, v, cap // 4, cap // 4, o, l, 1.0, stream=s)
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
    pat = AC.pattern("long4")
    D, Dv, scale = 32, 48, 0.25
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "wide", scale)
    dQ, dK, dV = (to_device(X, F32) for X in (Q, K, V))
    plan = AC.make_plan(pat)
    bufO, dO = filled(pat[0] * Dv)
    bufL, dL = filled(pat[0])
    torch.cuda.synchronize()
    caught = []

    def launch(s, dv=Dv, v=dV):
        plan.attention(dQ.data_ptr(), dK.data_ptr(), v.data_ptr(), D, dv, dO.data_ptr(), dL.data_ptr(), scale, stream=s)

    def refused(s):
        dL.zero_()
        with pytest.raises(bsmr.BsmrError) as ei:
            launch(s)
        caught.append(ei.value)

    g = _capture(torch, refused)  # ends normally: the refused launch did not invalidate the capture
    assert caught[0].status == bsmr.NOT_PREPARED
    assert "bsmr_attention: stream is capturing" in str(caught[0]) and "bsmr_plan_prepare_attention first" in str(caught[0])
    g.replay()
    torch.cuda.synchronize()
    assert (dL.cpu().numpy() == 0).all()
    assert (bufO.cpu().numpy().view(np.uint32) == FILL_BITS).all()
    assert not plan.attention_prepared(D, Dv)

    plan.prepare_attention(D, Dv)
    assert plan.attention_prepared(D, Dv) and plan.attention_prepared(D, 16)
    assert not plan.attention_prepared(D, 64), "the scratch of Dv = 48 does not hold the partials of Dv = 64"
    g = _capture(torch, launch)
    dO.fill_(float("nan"))
    dL.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    O = bufO.cpu().numpy()[:pat[0] * Dv].reshape(-1, Dv)
    L = bufL.cpu().numpy()[:pat[0]]
    direct = AC.make_plan(pat)
    O1, L1 = AC.attention_once(direct, Q, K, V, scale, dev=(dQ, dK, dV))
    assert _same_bits(O, O1) and _same_bits(L, L1), "the replay differs from the direct launch"
    assert (bufO.cpu().numpy()[pat[0] * Dv:].view(np.uint32) == FILL_BITS).all()
    # a larger Dv on the capturing stream is refused; prepare grows the scratch and keeps the lists
    V64 = AC.signed_data(pat[1] * 64, 9).reshape(-1, 64)
    dV64 = to_device(V64, F32)
    buf64, dO64 = filled(pat[0] * 64)
    torch.cuda.synchronize()

    def refused64(s):
        with pytest.raises(bsmr.BsmrError) as ei:
            plan.attention(dQ.data_ptr(), dK.data_ptr(), dV64.data_ptr(), D, 64, dO64.data_ptr(), 0, scale, stream=s)
        caught.append(ei.value)

    _capture(torch, refused64)
    assert caught[1].status == bsmr.NOT_PREPARED
    stats = plan.attention_stats()
    plan.prepare_attention(D, 64)
    assert plan.attention_prepared(D, 64) and plan.attention_prepared(D, Dv) and plan.attention_stats() == stats
    O2, _ = AC.attention_once(plan, Q, K, V, scale, dev=(dQ, dK, dV))
    assert _same_bits(O2, O1), "a grown scratch changed the result at the smaller Dv"
