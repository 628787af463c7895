"""GPU: bsmr_attention_heads and bsmr_attention_backward_heads with a head stride past 2^32 bytes, in
the spirit of tests/test_gpu_far_attention_bwd.py: a small pattern, H = 2, fp32 D = Dv = 64, and
slice 1 of an operand 4 GiB + 256 bytes behind slice 0 inside one torch.empty of 4 GiB and a little
(never filled: only the used rows are written). First every input is far and the outputs dense, then
the inputs dense and O (forward) or GQ, GK and GV (backward) far. Selector and flat data must come
out bit for bit, which they cannot with a slice base that wraps at 32 bits; the words behind each
far output slice hold FILL_BITS before and after. Skips cleanly when the allocation is refused.
"""
import numpy as np
import pytest

import attention_heads_cases as HC
from bsmr import F32
from gpu_util import torch_cuda

pytestmark = pytest.mark.gpu
NAME, B, H, D, DV = "long4", 1, 2, 64, 64
FAR = (1 << 30) + 64  # head stride in fp32 elements: 4 GiB + 256 bytes
SCALE = 0.125


def _far_buffer(rows, W):
    """(buffer, (1, 2, rows, W) view with head stride FAR); the words behind each slice hold FILL_BITS."""
    torch = torch_cuda()
    try:
        buf = torch.empty(FAR + rows * W + HC.GUARD, dtype=torch.float32, device="cuda")
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"no room for a 4 GiB operand: {str(e).splitlines()[0]}")
    for h in range(H):
        buf[h * FAR + rows * W:h * FAR + rows * W + HC.GUARD].view(torch.int32).fill_(HC.FILL_BITS)
    return buf, torch.as_strided(buf, (B, H, rows, W), (0, FAR, W, 1))


def _far_input(X):
    """X (2, rows, W) fp32 on the host as a far device view."""
    torch = torch_cuda()
    buf, view = _far_buffer(X.shape[1], X.shape[2])
    view.copy_(torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda().view(view.shape))
    return view


def _read_far(buf, view, what):
    rows, W = view.shape[2], view.shape[3]
    for h in range(H):
        g = buf[h * FAR + rows * W:h * FAR + rows * W + HC.GUARD].cpu().numpy().view(np.uint32)
        assert (g == HC.FILL_BITS).all(), f"{what}: a store behind slice {h}"
    return view.cpu().numpy().reshape(H, rows, W)


def _dense(X):
    return HC.place_input(X, B, H, "bhmd", F32)


def test_far_head_stride_forward():
    torch = torch_cuda()
    plan = HC.plan_of(NAME)
    sl = [HC.forward_slice("selector", NAME, D, DV, F32, SCALE, sq, skv) for sq, skv in HC.seeds(B, H, "bhmd")]
    s = torch.cuda.current_stream().cuda_stream
    # far inputs, dense O
    dev = tuple(_far_input(HC.stack(sl, k)) for k in ("Q", "K", "V"))
    assert all(t.stride(1) * 4 > 1 << 32 for t in dev)
    O, L = HC.heads_forward_once(plan, sl, B, H, "bhmd", SCALE, dev=dev)
    HC.assert_slices_equal(O, [x["O"] for x in sl], "far inputs: O selector")
    HC.assert_slices_equal(L[:, :, None], [x["LSE"][:, None] for x in sl], "far inputs: LSE selector")
    del dev
    torch.cuda.empty_cache()
    # dense inputs, far O
    dev = HC.forward_inputs(sl, B, H, "bhmd", F32)
    buf, vO = _far_buffer(plan.M, DV)
    vO.view(torch.int32).fill_(HC.FILL_BITS)
    bufL, vL = HC.place_output(B, H, plan.M, 1, "bhmd")
    plan.attention_heads(B, H, *dev, D, DV, vO, bufL.data_ptr(), SCALE, stream=s)
    torch.cuda.synchronize()
    O = _read_far(buf, vO, "O")
    assert not (O.view(np.uint32) == HC.FILL_BITS).any(), "an element of the far O was never written"
    HC.assert_slices_equal(O, [x["O"] for x in sl], "far O selector")
    L = HC.read_output(bufL, vL, "LSE")
    HC.assert_slices_equal(L, [x["LSE"][:, None] for x in sl], "far O: LSE selector")
    del buf, vO
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", ["selector", "flat"])
def test_far_head_stride_backward(kind):
    torch = torch_cuda()
    plan = HC.plan_of(NAME)
    sl = [HC.backward_slice(kind, NAME, D, DV, F32, SCALE, sq, skv) for sq, skv in HC.seeds(B, H, "bhmd")]
    s = torch.cuda.current_stream().cuda_stream
    lse = _dense(HC.stack(sl, "LSE")[:, :, None])
    # far inputs (Q, K, V, O and GO), dense gradients
    dev = tuple(_far_input(HC.stack(sl, k)) for k in ("Q", "K", "V", "O", "GO")) + (lse,)
    got = HC.heads_backward_once(plan, sl, B, H, "bhmd", SCALE, dev=dev)
    for k in HC.OUTPUTS:
        HC.assert_slices_equal(got[k], [x[k] for x in sl], f"far inputs: {k} {kind}")
    del dev
    torch.cuda.empty_cache()
    # dense inputs, far gradients
    dev = HC.backward_inputs(sl, B, H, "bhmd", F32)
    shapes = dict(GQ=(plan.M, D), GK=(plan.N, D), GV=(plan.N, DV))
    outs = {k: _far_buffer(r, c) for k, (r, c) in shapes.items()}
    for _, v in outs.values():
        v.view(torch.int32).fill_(HC.FILL_BITS)
    plan.attention_backward_heads(B, H, *dev[:5], dev[5].data_ptr(), D, DV, outs["GQ"][1], outs["GK"][1], outs["GV"][1],
                                  SCALE, stream=s)
    torch.cuda.synchronize()
    for k in HC.OUTPUTS:
        Y = _read_far(*outs[k], k)
        assert not (Y.view(np.uint32) == HC.FILL_BITS).any(), f"an element of the far {k} was never written"
        HC.assert_slices_equal(Y, [x[k] for x in sl], f"far {k} {kind}")
    del outs
    torch.cuda.empty_cache()
