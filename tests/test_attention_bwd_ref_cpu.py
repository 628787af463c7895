"""CPU: tests/attention_bwd_cases.py checked against itself, so that the GPU tests of the fused
sparse attention backward stand on a reference, bounds and data sets that are known to tell a right
kernel from a subtly wrong one.

* the numpy-fp32 emulation of the documented order (backward_emulate over the library's own
  bsmr.spmm_lists) stays inside backward_bound on every pattern, transpose, signed set and dtype;
  the worst ratios are printed;
* the exactness claims themselves: on the selector and the flat data the fp32 emulation equals the
  float64 reference bit for bit, and summing every segment (and the partials) in a shuffled order
  gives the same bits;
* backward_ref equals a dense masked attention differentiated by torch in float64;
* every mutation of the emulation fails on at least one exact set;
* the lists the emulation uses give the counts bsmr_attention_backward_stats reports, by
  arithmetic on the list lengths; the constants come from bsmr.attention_backward_limits().
"""
import numpy as np
import pytest

import attention_bwd_cases as BC
import attention_cases as AC
import bsmr
import spmm_cases
from bsmr import BF16, F16, F32

CPU_SHAPES = [(F32, 32, 48), (F16, 32, 128), (BF16, 64, 64)]  # generic form, D != Dv both ways; a compile-time form
SIGNED = [("narrow", 1.0), ("wide", 0.125), ("wide", None)]  # None: 1 / sqrt(D)


def _what(name, dtype, D, Dv):
    return f"{name} {BC.DTYPE_NAME[dtype]} {D}x{Dv}"


def test_constants_and_patterns_come_from_the_library():
    lim = BC.limits()
    assert lim == bsmr.attention_backward_limits() and lim["max_row_bytes"] == AC.limits()["max_row_bytes"]
    assert lim["row_chunk"] >= 1 and lim["col_chunk"] >= 1
    assert (BC.C1, BC.C2, BC.C3) == (2.0, 1.0, 3.0)
    for name, lens, c in (("long4", AC.row_lengths(BC.pattern("long4")), lim["row_chunk"]),
                          ("long4_T", BC.col_lengths(BC.pattern("long4_T")), lim["col_chunk"])):
        assert lens.max() == 4 * c + 3
        for n in (0, 1, c - 1, c, c + 1, 2 * c, 2 * c + 1):
            assert (lens == n).any(), (name, n)
    assert set(range(272)) <= set(BC.col_lengths(BC.pattern("staircase_T")).tolist())
    assert BC.col_lengths(BC.pattern("hub_T")).max() == 2048
    assert (BC.col_lengths(BC.pattern("empty_T")) == 0).any() and (BC.col_lengths(BC.pattern("empty")) == 0).any()
    for name in AC.PATTERNS:
        M, N, rp, ci = AC.pattern(name)
        Mt, Nt, rpt, cit = BC.pattern(name + "_T")
        dense = np.zeros((M, N), bool)
        dense[spmm_cases.entry_rows(M, rp), ci] = True
        denseT = np.zeros((Mt, Nt), bool)
        denseT[spmm_cases.entry_rows(Mt, rpt), cit] = True
        assert (dense.T == denseT).all() and len(ci) == len(cit)


@pytest.mark.parametrize("name", BC.PATTERNS)
def test_lists_give_the_stats(name):
    pat = BC.pattern(name)
    M, N, rp, ci = pat
    lim = BC.limits()
    want = BC.expected_stats(pat, 32, 48)
    for side, key in ((1, "row"), (2, "col")):
        segs, src, _ = bsmr.spmm_lists(M, N, rp, ci, side, lim[key + "_chunk"])
        count, part = segs[:, 2].astype(np.int64), segs[:, 3]
        split = part != bsmr.SPMM_DIRECT
        lens = np.bincount(segs[:, 0], weights=count, minlength=(M, N)[side - 1]).astype(np.int64)
        assert len(segs) == want[key + "_segments"] and int(split.sum()) == want[key + "_partials"]
        assert len(np.unique(segs[split, 0])) == want[key + "_split"] and int(lens.max()) == want[key + "_max"]
        assert count.max(initial=0) <= lim[key + "_chunk"] and count.sum() == len(ci)
    assert want["row_scratch_bytes"] == 4 * 32 * want["row_partials"]
    assert want["col_scratch_bytes"] == 4 * (32 + 48) * want["col_partials"] and want["delta_bytes"] == 4 * M


@pytest.mark.parametrize("dtype,D,Dv", CPU_SHAPES, ids=lambda x: str(x))
@pytest.mark.parametrize("name", BC.PATTERNS)
def test_emulation_stays_inside_the_bound(name, dtype, D, Dv):
    pat = BC.pattern(name)
    for kind, scale in SIGNED:
        scale = D ** -0.5 if scale is None else scale
        Q, K, V, O, GO, LSE, opscale, _ = BC.signed_inputs(pat, D, Dv, kind, scale, dtype)
        ref = BC.backward_ref(pat, Q, K, V, O, GO, LSE, scale, dtype)
        got = BC.backward_emulate(pat, Q, K, V, O, GO, LSE, scale, dtype)
        BC.check_bound(got, ref, f"emulation {_what(name, dtype, D, Dv)} {kind} scale {scale:.4f}", opscale)


def _exact_sets(pat, D, Dv, dtype):
    """(label, inputs, scale) of both exact sets."""
    for scale in BC.SCALES_EXACT:
        for order in ("random", "ascending", "descending"):
            yield f"selector {order} scale {scale}", BC.selector_inputs(pat, D, Dv, order, scale, dtype)[:6], scale
        yield f"flat scale {scale}", BC.flat_inputs(pat, D, Dv, dtype), scale


@pytest.mark.parametrize("dtype,D,Dv", CPU_SHAPES, ids=lambda x: str(x))
@pytest.mark.parametrize("name", BC.PATTERNS)
def test_exact_sets_are_exact_in_any_order(name, dtype, D, Dv):
    pat = BC.pattern(name)
    for label, inputs, scale in _exact_sets(pat, D, Dv, dtype):
        what = f"{_what(name, dtype, D, Dv)} {label}"
        ref = BC.backward_ref(pat, *inputs, scale, dtype)
        got = BC.backward_emulate(pat, *inputs, scale, dtype)
        BC.check_exact_all(got, ref, what)
        again = BC.backward_emulate(pat, *inputs, scale, dtype, shuffle=np.random.default_rng(3))
        assert BC.same_bits(got, again), f"{what}: a shuffled summation order changed the bits"
        if label.startswith("selector"):
            assert (ref["GQ"] == 0).all() and (ref["GK"] == 0).all()
            assert set(np.unique(ref["w"]).tolist()) <= {0.0, 1.0}
        else:
            assert (ref["p"] == 0).all() and (ref["w"] == 1).all()
            assert np.abs(ref["gd"]).max(initial=0) <= 8 and np.abs(ref["GK"]).max() > 0 and np.abs(ref["GQ"]).max() > 0


def test_selector_expected_is_the_reference():
    pat = BC.pattern("zipf_shuffled")
    Q, K, V, O, GO, LSE, winner = BC.selector_inputs(pat, 32, 48, "random", 0.125)
    ref = BC.backward_ref(pat, Q, K, V, O, GO, LSE, 0.125)
    GQ, GK, GV = BC.selector_expected(pat, GO, winner, 32, 48)
    assert (ref["GQ"] == GQ).all() and (ref["GK"] == GK).all() and (ref["GV"] == GV).all()
    assert np.abs(GV).max() > 0


def test_the_reference_is_the_dense_masked_attention_differentiated():
    import torch
    pat = BC.pattern("empty")
    M, N, rp, ci = pat
    D, Dv, scale = 16, 32, 0.25
    Q, K, V, O32, GO, LSE32, _, fwd = BC.signed_inputs(pat, D, Dv, "wide", scale)
    # float64 O and LSE: the identity is exact only when they are the softmax's own
    ref = BC.backward_ref(pat, Q, K, V, fwd["O"], GO, fwd["LSE"], scale, keep64=True)
    mask = torch.zeros((M, N), dtype=torch.bool)
    mask[torch.from_numpy(spmm_cases.entry_rows(M, rp)), torch.from_numpy(np.asarray(ci, np.int64))] = True
    q, k, v = (torch.from_numpy(X.astype(np.float64)).requires_grad_() for X in (Q, K, V))
    s = (q @ k.T) * scale
    w = torch.where(mask, torch.exp(s - torch.from_numpy(np.where(np.isfinite(fwd["LSE"]), fwd["LSE"], 0.0))[:, None]),
                    torch.zeros((), dtype=torch.float64))
    w = w / torch.where(w.sum(1, keepdim=True) == 0, torch.ones((), dtype=torch.float64), w.sum(1, keepdim=True))
    o = w @ v
    o.backward(torch.from_numpy(GO.astype(np.float64)))
    for name, t in (("GQ", q), ("GK", k), ("GV", v)):
        err = np.abs(t.grad.numpy() - ref[name]).max()
        top = np.abs(ref[name]).max()
        print(f"dense-vs-ref {name}: {err:.3e} of {top:.3e}")
        assert err <= 1e-12 * max(top, 1.0), name
    assert np.abs(o.detach().numpy() - fwd["O"]).max() <= 1e-13
    # and the fp32 rounding of O and LSE moves the reference by no more than composed_bound allows for it
    ref32 = BC.backward_ref(pat, Q, K, V, O32, GO, LSE32, scale)
    for name in BC.OUTPUTS:
        assert np.abs(ref32[name] - ref[name]).max() <= 1e-5


@pytest.mark.parametrize("mutation", BC.MUTATIONS)
def test_every_mutation_fails_an_exact_set(mutation):
    caught = []
    for name, dtype, D, Dv in (("long4_T", F32, 32, 48), ("zipf_shuffled", BF16, 64, 64)):
        pat = BC.pattern(name)
        for label, inputs, scale in _exact_sets(pat, D, Dv, dtype):
            ref = BC.backward_ref(pat, *inputs, scale, dtype)
            got = BC.backward_emulate(pat, *inputs, scale, dtype, mutation=mutation)
            try:
                BC.check_exact_all(got, ref, label)
            except AssertionError:
                caught.append(f"{name} {label}")
    print(f"{mutation}: caught by {caught}")
    assert caught, f"{mutation} passes both exact sets"
