"""GPU: the fused sparse attention forward (bsmr_attention / Plan.attention) against the float64
reference of tests/attention_cases.py, on every pattern (every row length 0 .. 271, a hub row,
shuffled columns, empty rows, a row of 4 chunk + 3 entries) and every lane form: fp32 at (D, Dv) in
(16, 16), (32, 48), (64, 64), (48, 128), (256, 256), fp16 and bf16 at (64, 64), (32, 128), (512, 512).

* selector data: O equals the winning V row and LSE the winning score times scale, bit for bit,
  with the winner random, the row's last entry (ascending: the maximum grows in every segment)
  and its first (descending), at scale 1 and 0.125;
* signed data, narrow and wide scores at scale 1, 0.125 and 1 / sqrt(D): O and LSE inside
  attention_bound / lse_bound; the worst ratios are printed (DESIGN.md section 13 records them);
* fused against the composition bsmr_sddmm, bsmr_softmax, bsmr_spmm on the same device inputs:
  |O_fused - O_composed| <= attention_bound + composed_bound, both from the float64 reference;
* bitwise: two launches agree; a prepared and a lazily built plan agree; prepare_spmm(chunk = 64)
  and recolumn change nothing; O without an LSE output is O with one.
Every launch goes through attention_cases.attention_once: outputs pre-filled, guard zones behind
them, every element written.
"""
import functools

import numpy as np
import pytest

import attention_cases as AC
from bsmr import BF16, F16, F32
from gpu_util import to_device, torch_cuda

pytestmark = pytest.mark.gpu

CASES = ([(F32, D, Dv) for D, Dv in AC.SHAPES_F32] +
         [(dt, D, Dv) for dt in (F16, BF16) for D, Dv in AC.SHAPES_HALF])


def _id(case):
    return f"{AC.DTYPE_NAME[case[0]]}_{case[1]}x{case[2]}"


@functools.lru_cache(maxsize=None)
def _plan(name):
    return AC.make_plan(AC.pattern(name))


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("name", AC.PATTERNS)
def test_selector_data_is_exact(name, case):
    dtype, D, Dv = case
    pat, plan = AC.pattern(name), _plan(name)
    for order in ("random", "ascending", "descending"):
        Q, K, V, winner, pi, base = AC.selector(pat, D, Dv, order, dtype)
        dev = (to_device(Q, dtype), to_device(K, dtype), to_device(V, dtype))
        for scale in AC.SCALES_EXACT:
            O, LSE = AC.attention_once(plan, Q, K, V, scale, dtype, dev=dev)
            wantO, wantL = AC.selector_expected(V, winner, pi, base, scale, dtype)
            AC.check_exact(O, wantO, f"O {name} {_id(case)} {order} scale {scale}")
            AC.check_exact(LSE, wantL, f"LSE {name} {_id(case)} {order} scale {scale}")


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("name", AC.PATTERNS)
def test_signed_data_stays_inside_the_bound(name, case, kind):
    dtype, D, Dv = case
    pat, plan = AC.pattern(name), _plan(name)
    for scale in (1.0, 0.125, D ** -0.5):
        Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, kind, scale)
        ref = AC.attention_ref(pat, Q, K, V, scale, dtype)
        O, LSE = AC.attention_once(plan, Q, K, V, scale, dtype)
        AC.check_bound(O, LSE, ref, f"{name} {_id(case)} {kind} scale {scale:.4f}", opscale)


@pytest.mark.parametrize("case", [(F32, 64, 64), (F32, 32, 48), (BF16, 64, 64)], ids=_id)
@pytest.mark.parametrize("name", ["zipf_shuffled", "hub", "long4"])
def test_fused_agrees_with_the_composition(name, case):
    torch = torch_cuda()
    dtype, D, Dv = case
    pat, plan = AC.pattern(name), _plan(name)
    M, nnz = pat[0], len(pat[3])
    s = torch.cuda.current_stream().cuda_stream
    for kind, scale in (("narrow", 1.0), ("wide", D ** -0.5)):
        Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, kind, scale)
        dQ, dK, dV = to_device(Q, dtype), to_device(K, dtype), to_device(V, dtype)
        O, _ = AC.attention_once(plan, Q, K, V, scale, dtype, dev=(dQ, dK, dV))
        P, W = (torch.empty(nnz, dtype=torch.float32, device="cuda") for _ in range(2))
        Oc = torch.empty((M, Dv), dtype=torch.float32, device="cuda")
        plan.sddmm(dQ.data_ptr(), dK.data_ptr(), D, P.data_ptr(), stream=s, dtype=dtype)
        plan.softmax(P.data_ptr(), W.data_ptr(), scale, stream=s)
        plan.spmm(W.data_ptr(), dV.data_ptr(), Dv, Oc.data_ptr(), stream=s, dtype=dtype)
        torch.cuda.synchronize()
        ref = AC.attention_ref(pat, Q, K, V, scale, dtype)
        bound = AC.attention_bound(ref, opscale) + AC.composed_bound(ref, opscale)
        diff = np.abs(O.astype(np.float64) - Oc.cpu().numpy().astype(np.float64))
        ratio = float((diff / bound).max())
        print(f"RATIO attention fused-vs-composed {ratio:.4f} {name} {_id(case)} {kind}")
        assert ratio <= 1.0, f"{name} {_id(case)} {kind}: |O_fused - O_composed| / (sum of bounds) = {ratio:.3f}"


@pytest.mark.parametrize("case", [(F32, 64, 64), (F32, 32, 48), (F16, 32, 128), (BF16, 512, 512)], ids=_id)
@pytest.mark.parametrize("name", ["staircase", "long4", "zipf_shuffled"])
def test_bitwise_reproducible(name, case):
    dtype, D, Dv = case
    pat = AC.pattern(name)
    scale = D ** -0.5
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "wide", scale)
    dev = (to_device(Q, dtype), to_device(K, dtype), to_device(V, dtype))
    lazy = AC.make_plan(pat)
    assert not lazy.attention_prepared(D, Dv)
    O, LSE = AC.attention_once(lazy, Q, K, V, scale, dtype, dev=dev)
    assert lazy.attention_prepared(D, Dv)
    stats = lazy.attention_stats()

    def same(what, plan, lse=True):
        O2, LSE2 = AC.attention_once(plan, Q, K, V, scale, dtype, lse=lse, dev=dev)
        assert _same_bits(O, O2), f"{what}: O differs"
        assert not lse or _same_bits(LSE, LSE2), f"{what}: LSE differs"

    same("second launch", lazy)
    same("no LSE output", lazy, lse=False)
    prepared = AC.make_plan(pat)
    prepared.prepare_attention(D, Dv)
    assert prepared.attention_prepared(D, Dv) and prepared.attention_stats() == stats
    same("prepared plan", prepared)
    lazy.prepare_spmm(Dv, 3, 64)
    assert lazy.spmm_stats(1)["chunk"] == 64 and lazy.attention_stats() == stats
    same("after prepare_spmm(chunk = 64)", lazy)
    lazy.recolumn(0.6)
    assert lazy.attention_prepared(D, Dv) and lazy.attention_stats() == stats
    same("after recolumn", lazy)
