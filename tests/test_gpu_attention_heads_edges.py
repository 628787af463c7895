"""GPU: edges of the fused sparse attention over batch and heads (bsmr_attention_heads,
bsmr_attention_backward_heads).

* guard zones: every launch goes through attention_heads_cases, whose outputs are pre-filled with
  FILL_BITS and padded: every element of every slice is written (empty rows and columns as exact
  zeros), nothing behind the last element, and the padding between the rows of a padded output is
  untouched;
* a NaN placed in one K row of one slice changes only the rows that the CSR names in that slice:
  every other slice, and every other row of that slice, is bit-equal to the clean run;
* every error code of the header contract, with the pre-filled outputs untouched and nothing built;
* graph capture: a plan prepared for one slice refuses Z = 3 on a capturing stream with
  BSMR_ERR_NOT_PREPARED and the capture stays usable; after prepare_attention_heads(.., 3) the plan's
  first launch is captured and its replay is bit-equal to the eager run;
* attention_heads_prepared is monotone in slices, and attention_prepared(D, Dv) returns as before on
  a plan that was only prepared for one slice;
* a prepare whose scratch the device refuses (the largest legal slice count) is an error that leaves
  the plan prepared for exactly what it held and the next launch right; the backward's scratch bytes
  (its stats; the forward reports none) do not shrink.
"""
import numpy as np
import pytest

import attention_bwd_cases as BC
import attention_heads_cases as HC
import bsmr
from bsmr import BF16, F16, F32
from gpu_util import torch_cuda

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 6
SCALE = 0.25


def _slices(fn, name, D, Dv, dtype, B, H, layout="bhmd", kind="signed", scale=SCALE):
    return [fn(kind, name, D, Dv, dtype, scale, sq, skv) for sq, skv in HC.seeds(B, H, layout)]


@pytest.mark.parametrize("layout", ["bmhd", "padded"])
@pytest.mark.parametrize("name", ["empty", "empty_T"])
def test_every_element_written_and_padding_untouched(name, layout):
    """(read_output holds every launch to the guard zones and the padding; here the destinations
    without entries, which only a store of zeros reaches.)"""
    pat = BC.pattern(name)
    plan = HC.plan_of(name)
    B, H, D, Dv = 2, 2, 32, 48
    rows0, cols0 = BC.AC.row_lengths(pat) == 0, BC.col_lengths(pat) == 0
    assert rows0.any() and cols0.any()
    O, L = HC.heads_forward_once(plan, _slices(HC.forward_slice, name, D, Dv, F32, B, H), B, H, layout, SCALE)
    assert (O[:, rows0].view(np.uint32) == 0).all() and (L[:, rows0] == -np.inf).all()
    got = HC.heads_backward_once(plan, _slices(HC.backward_slice, name, D, Dv, F32, B, H), B, H, layout, SCALE)
    assert (got["GQ"][:, rows0].view(np.uint32) == 0).all(), "an empty row of GQ is not +0"
    assert (got["GK"][:, cols0].view(np.uint32) == 0).all() and (got["GV"][:, cols0].view(np.uint32) == 0).all()
    assert all(np.isfinite(got[k]).all() for k in HC.OUTPUTS) and np.isfinite(O).all()


@pytest.mark.parametrize("dtype,D,Dv", [(F32, 32, 48), (F16, 64, 64)])
@pytest.mark.parametrize("layout", ["bhmd", "bmhd"])
def test_nan_in_one_k_row_of_one_slice_stays_there(layout, dtype, D, Dv):
    name, B, H, bad = "long4", 2, 2, 1
    pat = BC.pattern(name)
    M, N, rp, ci = pat
    plan = HC.plan_of(name)
    rows, cols = BC.AC.entry_rows(pat), np.asarray(ci, np.int64)
    refs = np.bincount(ci, minlength=N)
    target = int(np.nonzero((refs > 1) & (refs < (BC.AC.row_lengths(pat) > 0).sum()))[0][-1])
    hit_rows = np.zeros(M, bool)
    hit_rows[rows[cols == target]] = True
    hit_cols = np.zeros(N, bool)
    hit_cols[target] = True
    assert hit_rows.any() and not hit_rows.all()

    def poisoned(slices):
        out = [dict(s) for s in slices]
        K = out[bad]["K"].copy()
        K[target] = np.nan
        out[bad]["K"] = K
        return out

    fs = _slices(HC.forward_slice, name, D, Dv, dtype, B, H)
    clean = HC.heads_forward_once(plan, fs, B, H, layout, SCALE, dtype)
    got = HC.heads_forward_once(plan, poisoned(fs), B, H, layout, SCALE, dtype)
    for z in range(B * H):
        keep = ~hit_rows if z == bad else np.ones(M, bool)
        assert HC.bits_equal(got[0][z][keep], clean[0][z][keep]), f"O of slice {z} changed outside the named rows"
        assert HC.bits_equal(got[1][z][keep], clean[1][z][keep]), f"LSE of slice {z} changed outside the named rows"
    assert np.isnan(got[0][bad][hit_rows]).all() and np.isnan(got[1][bad][hit_rows]).all()

    bs = _slices(HC.backward_slice, name, D, Dv, dtype, B, H)
    clean = HC.heads_backward_once(plan, bs, B, H, layout, SCALE, dtype)
    got = HC.heads_backward_once(plan, poisoned(bs), B, H, layout, SCALE, dtype)
    for z in range(B * H):
        for k, hit in (("GQ", hit_rows), ("GK", hit_cols), ("GV", hit_cols)):
            keep = ~hit if z == bad else np.ones(len(hit), bool)
            assert HC.bits_equal(got[k][z][keep], clean[k][z][keep]), f"{k} of slice {z} changed outside the named rows"
    assert np.isnan(got["GQ"][bad][hit_rows]).all() and np.isnan(got["GK"][bad][hit_cols]).all()
    assert np.isnan(got["GV"][bad][hit_cols]).all()


def _status(fn, *a, **kw):
    with pytest.raises(bsmr.BsmrError) as ei:
        fn(*a, **kw)
    return ei.value.status, str(ei.value)


def test_errors_leave_the_outputs_untouched():
    torch = torch_cuda()
    name, B, H, D, Dv = "long4", 2, 3, 64, 64
    pat = BC.pattern(name)
    M, N = pat[0], pat[1]
    plan = BC.make_plan(pat)
    s = torch.cuda.current_stream().cuda_stream
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    W = 256  # room for the largest legal rows
    tQ, tK, tV, tO, tGO, tL = z(B, H, M, W), z(B, H, N, W), z(B, H, N, W), z(B, H, M, W), z(B, H, M, W), z(B, H, M)
    outs = {k: HC.place_output(B, H, r, W, "bhmd") for k, r in (("O", M), ("GQ", M), ("GK", N), ("GV", N))}
    bufL, _ = HC.place_output(B, H, M, 1, "bhmd")
    op = lambda t, w=D: bsmr.AttentionOperand.of(t[..., :w])  # noqa: E731
    Op = bsmr.AttentionOperand

    def fwd(Q=None, K=None, V=None, O=None, lse=None, batches=B, heads=H, D_=D, Dv_=Dv, scale=1.0, dtype=F32):
        return _status(plan.attention_heads, batches, heads, Q or op(tQ), K or op(tK), V or op(tV, Dv), D_, Dv_,
                       O or op(outs["O"][1], Dv), bufL.data_ptr() if lse is None else lse, scale, stream=s, dtype=dtype)

    def bwd(Q=None, K=None, V=None, O=None, GO=None, lse=None, G=None, batches=B, heads=H, D_=D, Dv_=Dv, scale=1.0,
            dtype=F32):
        G = G or (op(outs["GQ"][1]), op(outs["GK"][1]), op(outs["GV"][1], Dv))
        return _status(plan.attention_backward_heads, batches, heads, Q or op(tQ), K or op(tK), V or op(tV, Dv),
                       O or op(tO, Dv), GO or op(tGO, Dv), tL.data_ptr() if lse is None else lse, D_, Dv_, G[0], G[1], G[2],
                       scale, stream=s, dtype=dtype)

    def moved(o, **kw):
        vals = dict(ptr=o.ptr, batch=o.batch, head=o.head, row=o.row)
        vals.update(kw)
        return Op(vals["ptr"], vals["batch"], vals["head"], vals["row"])

    for call in (fwd, bwd):
        for scale in (0.0, -1.0, float("nan"), float("inf"), 3e38):
            st, msg = call(scale=scale)
            assert st == INVALID and "scale" in msg, (scale, msg)
        for batches, heads in ((0, H), (B, 0), (bsmr.ATTENTION_MAX_BATCHES + 1, H), (B, bsmr.ATTENTION_MAX_HEADS + 1)):
            st, msg = call(batches=batches, heads=heads)
            assert st == INVALID and "batches" in msg, (batches, heads, msg)
        q = op(tQ)
        for bad, word in ((moved(q, ptr=0), "null device pointer"), (moved(q, ptr=q.ptr + 4), "aligned"),
                          (moved(q, row=q.row + 2), "row stride"), (moved(q, row=D - 16), "below the row width"),
                          (moved(q, head=q.head + 1), "head stride"), (moved(q, batch=1 << 62), "64 bits")):
            st, msg = call(Q=bad)
            assert st == INVALID and word in msg and ": Q: " in msg, msg
        for key in ("K", "V"):
            st, msg = call(**{key: moved(op(tK), ptr=op(tK).ptr + 8)})
            assert st == INVALID and f": {key}: " in msg, msg
        cap = BC.limits()["max_row_bytes"]
        bad_dims = [(F32, 0, 64), (F32, 64, 0), (F32, 24, 64), (F32, 64, 40), (F32, cap // 4 + 16, 64),
                    (F32, 64, cap // 4 + 16), (F16, 48, 64), (BF16, 64, 40), (F16, 16, 64), (BF16, cap // 2 + 32, 64),
                    (3, 64, 64)]
        for dtype, d, dv in bad_dims:
            st, msg = call(D_=d, Dv_=dv, dtype=dtype)
            assert st == UNSUPPORTED, (dtype, d, dv, msg)
    # the outputs: a stride of 0, an overlap, a misaligned pointer
    o = op(outs["O"][1], Dv)
    for bad in (moved(o, head=0), moved(o, batch=0), moved(o, head=o.row * (M - 1)), moved(o, ptr=o.ptr + 8),
                moved(o, row=Dv - 16)):
        st, msg = fwd(O=bad)
        assert st == INVALID and ": O: " in msg, msg
    assert fwd(lse=bufL.data_ptr() + 2)[0] == INVALID
    g = (op(outs["GQ"][1]), op(outs["GK"][1]), op(outs["GV"][1], Dv))
    for i, key in enumerate(HC.OUTPUTS):
        for bad in (moved(g[i], head=0), moved(g[i], head=g[i].row * 2), moved(g[i], ptr=g[i].ptr + 4)):
            G = list(g)
            G[i] = bad
            st, msg = bwd(G=G)
            assert st == INVALID and f": {key}: " in msg, msg
    st, msg = bwd(G=(None, None, None))
    assert st == INVALID and "all null" in msg
    assert bwd(lse=tL.data_ptr() + 2)[0] == INVALID
    for key in ("O", "GO"):
        st, msg = bwd(**{key: moved(op(tO, Dv), row=Dv - 16)})
        assert st == INVALID and f": {key}: " in msg, msg
    # null plan, null operands, null LSE of the backward: straight through the library
    L = bsmr.lib()
    r = [bsmr.C.byref(x) for x in (op(tQ), op(tK), op(tV, Dv), o, op(tGO, Dv)) + g]
    assert L.bsmr_attention_heads(None, B, H, r[0], r[1], r[2], D, Dv, F32, 1.0, r[3], None, None) == INVALID
    assert L.bsmr_attention_backward_heads(None, B, H, *r[:5], tL.data_ptr(), D, Dv, F32, 1.0, *r[5:], None) == INVALID
    for i in range(4):
        a = list(r[:4])
        a[i] = None
        assert L.bsmr_attention_heads(plan.h, B, H, a[0], a[1], a[2], D, Dv, F32, 1.0, a[3], None, None) == INVALID, i
    for i in range(5):
        a = list(r[:5])
        a[i] = None
        assert L.bsmr_attention_backward_heads(plan.h, B, H, *a, tL.data_ptr(), D, Dv, F32, 1.0, *r[5:], None) == INVALID, i
    assert L.bsmr_attention_backward_heads(plan.h, B, H, *r[:5], None, D, Dv, F32, 1.0, *r[5:], None) == INVALID
    torch.cuda.synchronize()
    for k, (buf, _) in outs.items():
        assert (buf.cpu().numpy().view(np.uint32) == HC.FILL_BITS).all(), f"a refused call wrote {k}"
    assert (bufL.cpu().numpy().view(np.uint32) == HC.FILL_BITS).all(), "a refused call wrote LSE"
    assert not plan.attention_heads_prepared(D, Dv, 1) and not plan.attention_backward_heads_prepared(D, Dv, 1)
    assert plan.attention_backward_stats() == BC.expected_stats(pat, built=False)
    for prep in (plan.prepare_attention_heads, plan.prepare_attention_backward_heads):
        assert _status(prep, 24, 64, 2)[0] == UNSUPPORTED
        assert _status(prep, 64, 64, 0)[0] == INVALID
    assert not plan.attention_heads_prepared(64, 64, 0) and not plan.attention_backward_heads_prepared(64, 64, 0)
    # the largest legal rows pass
    cap = BC.limits()["max_row_bytes"]
    plan.attention_heads(B, H, op(tQ, W), op(tK, W), op(tV, W), cap // 4, cap // 4, op(outs["O"][1], W), 0, 1.0, stream=s)
    torch.cuda.synchronize()


def _capture(torch, fn):
    """fn(stream) recorded into a graph on a side stream (a plain chain of nodes)."""
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(side.cuda_stream)
    return g


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_capture_needs_a_plan_prepared_for_the_slices(direction):
    torch = torch_cuda()
    name = "long4" if direction == "forward" else "long4_T"
    pat = BC.pattern(name)
    M, N = pat[0], pat[1]
    B, H, D, Dv, layout = 1, 3, 32, 48, "bmhd"
    Z = B * H
    plan = BC.make_plan(pat)
    fwd = direction == "forward"
    if fwd:
        sl = _slices(HC.forward_slice, name, D, Dv, F32, B, H)
        dev = HC.forward_inputs(sl, B, H, layout, F32)
        shapes = dict(O=(M, Dv), LSE=(M, 1))
        once = lambda p: dict(zip(("O", "LSE"), HC.heads_forward_once(p, sl, B, H, layout, SCALE, dev=dev)))  # noqa: E731
        prepare, prepared, single = plan.prepare_attention_heads, plan.attention_heads_prepared, plan.prepare_attention
        old_prepared = plan.attention_prepared
    else:
        sl = _slices(HC.backward_slice, name, D, Dv, F32, B, H)
        dev = HC.backward_inputs(sl, B, H, layout, F32)
        shapes = dict(GQ=(M, D), GK=(N, D), GV=(N, Dv))
        once = lambda p: HC.heads_backward_once(p, sl, B, H, layout, SCALE, dev=dev)  # noqa: E731
        prepare, prepared = plan.prepare_attention_backward_heads, plan.attention_backward_heads_prepared
        single, old_prepared = plan.prepare_attention_backward, plan.attention_backward_prepared
    outs = {k: HC.place_output(B, H, r, c, "bhmd" if k == "LSE" else layout) for k, (r, c) in shapes.items()}
    marker = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    caught = []

    def launch(s):
        if fwd:
            plan.attention_heads(B, H, *dev, D, Dv, outs["O"][1], outs["LSE"][0].data_ptr(), SCALE, stream=s)
        else:
            plan.attention_backward_heads(B, H, *dev[:5], dev[5].data_ptr(), D, Dv, outs["GQ"][1], outs["GK"][1],
                                          outs["GV"][1], SCALE, stream=s)

    def refused(s):
        marker.zero_()
        with pytest.raises(bsmr.BsmrError) as ei:
            launch(s)
        caught.append(ei.value)

    single(D, Dv)  # one slice only
    assert old_prepared(D, Dv) and prepared(D, Dv, 1) and not prepared(D, Dv, Z)
    g = _capture(torch, refused)  # ends normally: the refused launch did not invalidate the capture
    assert caught[0].status == bsmr.NOT_PREPARED
    who = "bsmr_attention_heads" if fwd else "bsmr_attention_backward_heads"
    assert f"{who}: stream is capturing" in str(caught[0]) and f"{Z} slices" in str(caught[0])
    assert ("bsmr_plan_prepare_attention_heads first" if fwd else "bsmr_plan_prepare_attention_backward_heads first") in str(
        caught[0])
    marker.fill_(1)
    g.replay()
    torch.cuda.synchronize()
    assert float(marker.cpu()[0]) == 0, "the capture did not stay usable"
    for buf, _ in outs.values():
        assert (buf.cpu().numpy().view(np.uint32) == HC.FILL_BITS).all()
    assert old_prepared(D, Dv) and not prepared(D, Dv, Z), "a refused launch built something"

    prepare(D, Dv, Z)
    # monotone in slices; the single-slice question answers as before
    assert all(prepared(D, Dv, n) for n in range(1, Z + 1)) and not prepared(D, Dv, Z + 1)
    assert old_prepared(D, Dv) and prepared(D, 16, Z)
    assert not prepared(D, 64, Z), "the scratch of Dv = 48 does not hold the partials of Dv = 64"
    g = _capture(torch, launch)  # the plan's first launch
    eager = once(BC.make_plan(pat))
    for replay in (1, 2):
        for buf, _ in outs.values():
            buf.view(torch.int32).fill_(HC.FILL_BITS)
        g.replay()
        torch.cuda.synchronize()
        for k, (buf, view) in outs.items():
            Y = HC.read_output(buf, view, f"replay {replay} {k}")
            want = eager[k][:, :, None] if k == "LSE" else eager[k]
            assert HC.bits_equal(Y, want), f"replay {replay}: {k} differs from the eager run"
    prepare(D, Dv, 1)  # fewer slices keep the scratch
    assert prepared(D, Dv, Z)


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_a_refused_scratch_grow_leaves_the_plan_as_it_was(direction):
    """A prepare for more slices than the device has memory for (the largest legal count: terabytes of
    scratch) is an error; the plan stays prepared for what it held, is not prepared for more, and
    the next launch gives the bits of a fresh plan. The backward's stats report its scratch bytes,
    which must not shrink; the forward has no such figure, so there "kept" is what prepared() and the
    bit-equal launch show."""
    fwd = direction == "forward"
    name = "long4" if fwd else "long4_T"
    pat = BC.pattern(name)
    B, H, D, Dv, layout = 1, 2, 32, 48, "bhmd"
    Z = B * H
    huge = bsmr.ATTENTION_MAX_BATCHES * bsmr.ATTENTION_MAX_HEADS
    plan = BC.make_plan(pat)
    if fwd:
        prepare, prepared = plan.prepare_attention_heads, plan.attention_heads_prepared
        sl = _slices(HC.forward_slice, name, D, Dv, F32, B, H)
        once = lambda p: dict(zip(("O", "LSE"), HC.heads_forward_once(p, sl, B, H, layout, SCALE)))  # noqa: E731
        partials = BC.expected_stats(pat)["row_partials"]  # (the forward's lists are the backward's row lists)
        assert partials >= 8 and 4 * huge * partials * (Dv + 2) > 1 << 42  # at least 4 TiB of scratch
    else:
        prepare, prepared = plan.prepare_attention_backward_heads, plan.attention_backward_heads_prepared
        sl = _slices(HC.backward_slice, name, D, Dv, F32, B, H)
        once = lambda p: HC.heads_backward_once(p, sl, B, H, layout, SCALE)  # noqa: E731
        assert 4 * huge * pat[0] > 1 << 42  # delta alone: at least 4 TiB
    # a plan that never held anything: refused, and nothing is prepared
    st, msg = _status(prepare, D, Dv, huge)
    assert st not in (0, INVALID, UNSUPPORTED, bsmr.NOT_PREPARED), (st, msg)
    assert not prepared(D, Dv, huge) and not prepared(D, Dv, Z)
    prepare(D, Dv, Z)
    before = plan.attention_backward_stats()
    assert prepared(D, Dv, Z) and not prepared(D, Dv, Z + 1)
    st, msg = _status(prepare, D, Dv, huge)
    assert st not in (0, INVALID, UNSUPPORTED, bsmr.NOT_PREPARED), (st, msg)
    assert prepared(D, Dv, Z) and not prepared(D, Dv, Z + 1) and not prepared(D, Dv, huge)
    after = plan.attention_backward_stats()
    for k in ("row_scratch_bytes", "col_scratch_bytes", "delta_bytes"):
        assert after[k] >= before[k], f"{k} shrank after a refused grow"
    got, want = once(plan), once(BC.make_plan(pat))
    for k in want:
        assert HC.bits_equal(got[k], want[k]), f"{k} after a refused grow"
