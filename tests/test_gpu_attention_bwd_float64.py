"""GPU: the fused sparse attention backward (bsmr_attention_backward / Plan.attention_backward)
against the float64 reference of tests/attention_bwd_cases.py, on every pattern and its transpose
(both sides see every list length 0 .. 271, a 2048 hub, shuffled columns, empty destinations, lists
of chunk - 1 .. 4 chunk + 3) and every lane form: fp32 at (D, Dv) in (16, 16), (32, 48), (64, 64),
(48, 128), (256, 256), fp16 and bf16 at (64, 64), (32, 128), (512, 512).

* both exact sets bit for bit: selector (GQ = GK = 0, GV the winners' GO sums; winner random, last
  and first entry of the row; scale 1 and 0.125) and flat (every entry contributes to all three);
* signed data, narrow scores at scale 1 and wide ones at 1 / sqrt(D): GQ, GK and GV inside
  backward_bound; the worst ratios are printed (DESIGN.md section 14 records them);
* fused against the composed backward (attention's launch sequence on the same device inputs):
  within backward_bound + composed_bound, both from the float64 reference;
* bitwise, no tolerance: two launches; lazy against prepared; before and after prepare_spmm(chunk =
  64) and recolumn; every NULL-output combination against the full call; a forward launch between
  two backward launches (the scratches do not alias);
* attention_backward_stats equals what the list lengths give.
Every launch goes through attention_bwd_cases.backward_once: outputs pre-filled, guard zones behind
them, every element of a requested output written and none of the others.
"""
import functools
import itertools

import numpy as np
import pytest

import attention_bwd_cases as BC
import attention_cases as AC
from bsmr import BF16, F16, F32
from gpu_util import torch_cuda

pytestmark = pytest.mark.gpu

CASES = ([(F32, D, Dv) for D, Dv in BC.SHAPES_F32] +
         [(dt, D, Dv) for dt in (F16, BF16) for D, Dv in BC.SHAPES_HALF])


def _id(case):
    return f"{BC.DTYPE_NAME[case[0]]}_{case[1]}x{case[2]}"


@functools.lru_cache(maxsize=None)
def _plan(name):
    return BC.make_plan(BC.pattern(name))


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("name", BC.PATTERNS)
def test_selector_data_is_exact(name, case):
    dtype, D, Dv = case
    pat, plan = BC.pattern(name), _plan(name)
    for order in ("random", "ascending", "descending"):
        for scale in BC.SCALES_EXACT:
            Q, K, V, O, GO, LSE, winner = BC.selector_inputs(pat, D, Dv, order, scale, dtype)
            got = BC.backward_once(plan, Q, K, V, O, GO, LSE, scale, dtype)
            want = BC.selector_expected(pat, GO, winner, D, Dv)
            for k, w in zip(BC.OUTPUTS, want):
                BC.check_exact(got[k], w, f"{k} {name} {_id(case)} {order} scale {scale}")


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("name", BC.PATTERNS)
def test_flat_data_is_exact(name, case):
    dtype, D, Dv = case
    pat, plan = BC.pattern(name), _plan(name)
    inputs = BC.flat_inputs(pat, D, Dv, dtype)
    dev = BC.device_inputs(*inputs, dtype)
    for scale in (1.0, 0.125):
        ref = BC.backward_ref(pat, *inputs, scale, dtype)
        got = BC.backward_once(plan, *inputs, scale, dtype, dev=dev)
        BC.check_exact_all(got, ref, f"{name} {_id(case)} flat scale {scale}")


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("name", BC.PATTERNS)
def test_signed_data_stays_inside_the_bound(name, case):
    dtype, D, Dv = case
    pat, plan = BC.pattern(name), _plan(name)
    for kind, scale in (("narrow", 1.0), ("wide", D ** -0.5)):
        Q, K, V, O, GO, LSE, opscale, _ = BC.signed_inputs(pat, D, Dv, kind, scale, dtype)
        ref = BC.backward_ref(pat, Q, K, V, O, GO, LSE, scale, dtype)
        got = BC.backward_once(plan, Q, K, V, O, GO, LSE, scale, dtype)
        BC.check_bound(got, ref, f"{name} {_id(case)} {kind} scale {scale:.4f}", opscale)


def composed_backward(plan, dev, D, Dv, scale, dtype):
    """dict(GQ, GK, GV) (numpy fp32) of attention's backward launches on the device operands."""
    torch = torch_cuda()
    dQ, dK, dV, _, dGO, _ = dev
    s = torch.cuda.current_stream().cuda_stream
    vec = lambda: torch.empty(max(plan.nnz, 1), dtype=torch.float32, device="cuda")  # noqa: E731
    P, W, gW, gP = vec(), vec(), vec(), vec()
    gQ = torch.empty((plan.M, D), dtype=torch.float32, device="cuda")
    gK = torch.empty((plan.N, D), dtype=torch.float32, device="cuda")
    gV = torch.empty((plan.N, Dv), dtype=torch.float32, device="cuda")
    plan.sddmm(dQ.data_ptr(), dK.data_ptr(), D, P.data_ptr(), stream=s, dtype=dtype)
    plan.softmax(P.data_ptr(), W.data_ptr(), scale, stream=s)
    plan.sddmm(dGO.data_ptr(), dV.float().data_ptr(), Dv, gW.data_ptr(), stream=s)
    plan.spmm_t(W.data_ptr(), dGO.data_ptr(), Dv, gV.data_ptr(), stream=s)
    plan.softmax_backward(W.data_ptr(), gW.data_ptr(), gP.data_ptr(), scale, stream=s)
    plan.sddmm_backward(gP.data_ptr(), dQ.data_ptr(), dK.data_ptr(), D, gQ.data_ptr(), gK.data_ptr(), stream=s,
                        dtype=dtype)
    torch.cuda.synchronize()
    return dict(GQ=gQ.cpu().numpy(), GK=gK.cpu().numpy(), GV=gV.cpu().numpy())


@pytest.mark.parametrize("case", [(F32, 64, 64), (F32, 32, 48), (BF16, 64, 64)], ids=_id)
@pytest.mark.parametrize("name", ["zipf_shuffled", "hub", "long4_T"])
def test_fused_agrees_with_the_composed_backward(name, case):
    dtype, D, Dv = case
    pat, plan = BC.pattern(name), _plan(name)
    for kind, scale in (("narrow", 1.0), ("wide", D ** -0.5)):
        Q, K, V, O, GO, LSE, opscale, fwd = BC.signed_inputs(pat, D, Dv, kind, scale, dtype)
        dev = BC.device_inputs(Q, K, V, O, GO, LSE, dtype)
        got = BC.backward_once(plan, Q, K, V, O, GO, LSE, scale, dtype, dev=dev)
        comp = composed_backward(plan, dev, D, Dv, scale, dtype)
        ref = BC.backward_ref(pat, Q, K, V, O, GO, LSE, scale, dtype)
        fb, cb = BC.backward_bound(ref, opscale), BC.composed_bound(ref, fwd, opscale)
        for k in BC.OUTPUTS:
            diff = np.abs(got[k].astype(np.float64) - comp[k].astype(np.float64))
            ratio = AC._ratio(diff, fb[k] + cb[k])
            print(f"RATIO attention_bwd fused-vs-composed {k} {ratio:.4f} {name} {_id(case)} {kind}")
            assert ratio <= 1.0, f"{name} {_id(case)} {kind}: |{k}_fused - {k}_composed| / (sum of bounds) = {ratio:.3f}"


@pytest.mark.parametrize("case", [(F32, 64, 64), (F32, 32, 48), (F16, 32, 128), (BF16, 512, 512)], ids=_id)
@pytest.mark.parametrize("name", ["staircase", "long4", "long4_T", "zipf_shuffled"])
def test_bitwise_reproducible(name, case):
    torch = torch_cuda()
    dtype, D, Dv = case
    pat = BC.pattern(name)
    scale = D ** -0.5
    inputs = BC.signed_inputs(pat, D, Dv, "wide", scale, dtype)[:6]
    dev = BC.device_inputs(*inputs, dtype)
    lazy = BC.make_plan(pat)
    assert not lazy.attention_backward_prepared(D, Dv)
    assert lazy.attention_backward_stats() == BC.expected_stats(pat, built=False)
    first = BC.backward_once(lazy, *inputs, scale, dtype, dev=dev)
    assert lazy.attention_backward_prepared(D, Dv)
    stats = lazy.attention_backward_stats()
    assert stats == BC.expected_stats(pat, D, Dv), (stats, BC.expected_stats(pat, D, Dv))
    assert not lazy.attention_prepared(D, Dv) and lazy.attention_stats()["segments"] == 0, "the forward's state was touched"

    def same(what, plan, want=BC.OUTPUTS):
        again = BC.backward_once(plan, *inputs, scale, dtype, want=want, dev=dev)
        for k in want:
            assert (again[k].view(np.uint32) == first[k].view(np.uint32)).all(), f"{what}: {k} differs"

    same("second launch", lazy)
    for n in (1, 2):
        for want in itertools.combinations(BC.OUTPUTS, n):
            same(f"outputs {want} alone", lazy, want)
    prepared = BC.make_plan(pat)
    prepared.prepare_attention_backward(D, Dv)
    assert prepared.attention_backward_prepared(D, Dv) and prepared.attention_backward_stats() == stats
    same("prepared plan", prepared)
    # a forward launch between two backward launches: its lists are shared from here on, its scratch is its own
    dQ, dK, dV = dev[:3]
    fO = torch.empty((pat[0], Dv), dtype=torch.float32, device="cuda")
    lazy.attention(dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D, Dv, fO.data_ptr(), 0, scale,
                   stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    same("after a forward launch", lazy)
    shared = BC.make_plan(pat)
    shared.prepare_attention(D, Dv)
    fstats = shared.attention_stats()
    same("forward prepared first (shared row lists)", shared)
    assert shared.attention_stats() == fstats and shared.attention_backward_stats() == stats
    lazy.prepare_spmm(Dv, 3, 64)
    assert lazy.spmm_stats(2)["chunk"] == 64 and lazy.attention_backward_stats() == stats
    same("after prepare_spmm(chunk = 64)", lazy)
    lazy.recolumn(0.6)
    assert lazy.attention_backward_prepared(D, Dv) and lazy.attention_backward_stats() == stats
    same("after recolumn", lazy)
