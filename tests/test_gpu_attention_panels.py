"""GPU: the panel form of the fused attention forward on matrix instructions (bsmr_attention_panels,
DESIGN.md section 18), fp16 / bf16 at every compile-time (D, Dv) form, on the smallest patterns that
can break it: bit-exact selector data; O and LSE inside a derived bound of the float64 reference and
|O_panels - O_gather| inside the sum of the two paths' bounds; heads slices bit-equal to the
single-slice call; guard zones, NaN containment, refused shapes, graph capture; autograd end to end.

The bound of O is attention_cases.attention_bound plus what this path adds (panel_terms; derived in
section 18); that of LSE is lse_bound plus 3 s u: per step l is multiplied by an exponential within
2 u and the product rounds once (s the steps of the row's panel, u = 2^-24).
"""
import functools

import numpy as np
import pytest

import attention_cases as AC
import bsmr
from attention_cases import FILL_BITS, filled
from bsmr import BF16, F16, F32
from gpu_util import half_values, to_device, torch_cuda
from attention_panels_cases import block_mask

pytestmark = pytest.mark.gpu
UNSUPPORTED = 6
U = 2.0 ** -24
SHAPES = [(32, 32), (64, 128), (128, 64), (256, 256)]
FORMS = [pytest.param(dt, D, Dv, id=f"{AC.DTYPE_NAME[dt]}-{D}-{Dv}") for dt in (F16, BF16) for D, Dv in SHAPES]
PATTERNS = ["staircase37", "union_32_33", "empty_row_and_panel", "split", "hub", "block_mask"]


def _groups(groups, N):
    """Rows given as (count, columns) groups: `count` rows storing exactly `columns`."""
    lens = np.concatenate([[len(c)] * n for n, c in groups])
    ci = np.concatenate([np.tile(np.asarray(c, np.uint32), n) for n, c in groups])
    return len(lens), N, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32), ci.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def pattern(name):
    r = np.arange
    if name == "staircase37":  # M = 37: a short last panel; row i stores columns 0 .. i
        return _groups([(1, r(i + 1)) for i in range(37)], 40)
    if name == "union_32_33":  # one panel of exactly one full step, one of a step and a column
        return _groups([(16, r(32)), (16, r(40, 73))], 80)
    if name == "empty_row_and_panel":
        return _groups([(7, r(3, 23)), (1, []), (8, r(3, 23)), (16, [])], 32)
    if name == "split":  # a union of item_steps x 32 + 1 columns: two items, the second of one column
        n = bsmr.attention_panels_limits()["item_steps"] * 32 + 1
        return _groups([(16, r(n)), (5, r(7))], n + 3)
    return block_mask() if name == "block_mask" else AC.pattern(name)


@functools.lru_cache(maxsize=None)
def plan_of(name):
    return AC.make_plan(pattern(name))


@functools.lru_cache(maxsize=None)
def lists_of(name):
    """The host lists over the plan's own row order, and per row the steps of its panel."""
    M, N, rp, ci = pattern(name)
    rows, cols, masks, items, reds = bsmr.attention_panel_lists(M, N, rp, ci, plan_of(name).array("reorderedRows"))
    steps = np.zeros(M)
    np.add.at(steps, items[:, 0] // 16, items[:, 2])
    s = np.empty(M)
    s[rows] = steps[np.arange(M) // 16]
    return rows, cols, items, s


def once(plan, Q, K, V, scale, dtype, fn="attention_panels", dev=None):
    """(O, LSE) of one launch on host operands; both outputs start as FILL_BITS with a guard zone."""
    torch = torch_cuda()
    D, Dv = Q.shape[1], V.shape[1]
    dQ, dK, dV = dev or [to_device(X, dtype) for X in (Q, K, V)]
    bufO, dO = filled(plan.M * Dv)
    bufL, dL = filled(plan.M)
    getattr(plan, fn)(dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D, Dv, dO.data_ptr(), dL.data_ptr(), scale,
                      stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    hO, hL = bufO.cpu().numpy(), bufL.cpu().numpy()
    assert (hO[plan.M * Dv:].view(np.uint32) == FILL_BITS).all() and (hL[plan.M:].view(np.uint32) == FILL_BITS).all()
    assert not (hO[:plan.M * Dv].view(np.uint32) == FILL_BITS).any() and not (hL[:plan.M].view(np.uint32) == FILL_BITS).any()
    return hO[:plan.M * Dv].reshape(plan.M, Dv), hL[:plan.M]


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_selector_data_is_bit_exact(dtype, D, Dv, name):
    pat, plan = pattern(name), plan_of(name)
    for order, scale in (("random", 1.0), ("ascending", 0.125), ("descending", 1.0)):
        Q, K, V, winner, pi, base = AC.selector(pat, D, Dv, order, dtype)
        O, LSE = once(plan, Q, K, V, scale, dtype)
        wantO, wantL = AC.selector_expected(V, winner, pi, base, scale, dtype)
        AC.check_exact(O, wantO, f"O {name} {order}")
        AC.check_exact(LSE, wantL, f"LSE {name} {order}")
    st = plan.attention_panels_stats()
    assert st["items"] == len(lists_of(name)[2]) and st["panels"] == -(-pat[0] // 16)
    if name in ("split", "hub"):
        assert st["split_panels"] >= 1 and st["partials"] >= 2
    if name == "block_mask":
        assert st["fill_permille"] == 1000


def panel_terms(ref, dtype, s):
    """Per element of O, with A = sum W |V|: u_T A (weights rounded to the operand type), s u A (one
    rounded rescale per step) and for fp16 n 2^-25 max|V| (weights under the normal range)."""
    A = AC._weighted(ref, ref["W"])
    n = ref["lens"].astype(np.float64)[:, None]
    uT = 2.0 ** -11 if dtype == F16 else 2.0 ** -8
    return uT * A + s[:, None] * U * A + (n * 2.0 ** -25 * np.abs(ref["V"]).max() if dtype == F16 else 0.0)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_against_float64(dtype, D, Dv, name):
    pat, plan = pattern(name), plan_of(name)
    s = lists_of(name)[3]
    for kind, scale in (("narrow", 1.0), ("wide", 1.0), ("narrow", D ** -0.5), ("wide", D ** -0.5)):
        Q, K, V, opscale = AC.signed_inputs(pat, D, Dv, kind, scale)
        dev = [to_device(X, dtype) for X in (Q, K, V)]
        O, LSE = once(plan, Q, K, V, scale, dtype, dev=dev)
        Og, _ = once(plan, Q, K, V, scale, dtype, fn="attention", dev=dev)
        ref = AC.attention_ref(pat, Q, K, V, scale, dtype)
        gather = AC.attention_bound(ref, opscale)
        bound = gather + panel_terms(ref, dtype, s)
        live = ref["lens"] > 0
        ro = AC._ratio(np.abs(O - ref["O"]), bound)
        rl = AC._ratio(np.abs(LSE[live] - ref["LSE"][live]), (AC.lse_bound(ref, opscale) + 3 * s * U)[live])
        rg = AC._ratio(np.abs(O.astype(np.float64) - Og), bound + gather)
        print(f"RATIO attention_panels {AC.DTYPE_NAME[dtype]} {D} {Dv} {name} {kind} {scale:.4f}: O {ro:.4f} LSE {rl:.4f} "
              f"vs gather {rg:.4f}")
        assert (O[~live] == 0).all() and (LSE[~live] == -np.inf).all()
        assert ro <= 1.0 and rl <= 1.0 and rg <= 1.0, (kind, scale, ro, rl, rg)


@pytest.mark.parametrize("dtype,D,Dv", [(F16, 64, 128), (BF16, 32, 32)])
def test_heads_slices_equal_the_single_slice_call(dtype, D, Dv):
    torch = torch_cuda()
    name, B, H = "hub", 2, 3  # (split panels: a scratch per slice)
    pat, plan = pattern(name), plan_of(name)
    M, N = pat[0], pat[1]
    tdt = torch.float16 if dtype == F16 else torch.bfloat16
    data = lambda n, seed: torch.from_numpy(AC.signed_data(n, seed)).to(tdt).cuda()  # noqa: E731
    Q = data(B * M * H * D, 1).view(B, M, H, D).transpose(1, 2)  # a view of a (B, M, H D) projection
    K = data(B * N * D, 2).view(B, 1, N, D).expand(B, H, N, D)   # one K / V for all heads: head stride 0
    V = data(B * N * Dv, 3).view(B, 1, N, Dv).expand(B, H, N, Dv)
    O = torch.full((B, M, H, Dv), float("nan"), device="cuda").transpose(1, 2)
    L = torch.full((B, H, M), float("nan"), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    plan.attention_panels_heads(B, H, Q, K, V, D, Dv, O, L.data_ptr(), 0.25, stream=s, dtype=dtype)
    for b in range(B):
        for h in range(H):
            q, k, v = (X[b, h].contiguous() for X in (Q, K, V))
            o, l = torch.empty(M, Dv, device="cuda"), torch.empty(M, device="cuda")
            plan.attention_panels(q.data_ptr(), k.data_ptr(), v.data_ptr(), D, Dv, o.data_ptr(), l.data_ptr(), 0.25,
                                  stream=s, dtype=dtype)
            assert torch.equal(O[b, h], o) and torch.equal(L[b, h], l), (b, h)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_nan_stays_in_its_rows_and_panels(dtype):
    name, D, Dv = "hub", 64, 64
    pat, plan = pattern(name), plan_of(name)
    M, N, rp, ci = pat
    rows, cols, items, _ = lists_of(name)
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "narrow", 0.125)
    clean = once(plan, Q, K, V, 0.125, dtype)
    erows = AC.entry_rows(pat)
    j = int(ci[rp[5]])  # a column that a short row stores (the hub row stores it too)
    storing = np.zeros(M, bool)
    storing[erows[ci == j]] = True
    in_panel = np.zeros(M, bool)  # rows of the panels whose union holds j
    for row0, step0, nsteps, _ in items:
        if (cols[step0:step0 + nsteps] == j).any():
            in_panel[rows[row0:row0 + 16]] = True
    one_row = np.zeros(M, bool)
    one_row[5] = True
    for what, X, idx, must, may in (("Q", 0, 5, one_row, one_row), ("K", 1, j, storing, storing), ("V", 2, j, storing, in_panel)):
        ops = [Q.copy(), K.copy(), V.copy()]
        ops[X][idx, 3] = np.nan
        O, LSE = once(plan, *ops, 0.125, dtype)
        changed = (O.view(np.uint32) != clean[0].view(np.uint32)).any(axis=1)
        assert np.isnan(O[must]).any(axis=1).all() and not changed[~may].any(), what
        assert (np.isnan(LSE) == (must if what != "V" else False)).all(), what
        assert (LSE.view(np.uint32) == clean[1].view(np.uint32))[~must].all(), what
    assert not in_panel.all(), "the pattern must have a panel that does not hold the column"


def test_refused_shapes_and_capture():
    torch = torch_cuda()
    name, D, Dv = "split", 64, 32
    pat = pattern(name)
    plan = AC.make_plan(pat)  # a fresh plan: nothing prepared
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "narrow", 0.125)
    dQ, dK, dV = (to_device(X, F16) for X in (Q, K, V))
    bufO, dO = filled(plan.M * Dv)
    bufL, dL = filled(plan.M)

    def launch(s, D_=D, dt=F16):
        plan.attention_panels(dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D_, Dv, dO.data_ptr(), dL.data_ptr(), 0.125,
                              stream=s, dtype=dt)

    def status(s, **kw):
        with pytest.raises(bsmr.BsmrError) as ei:
            launch(s, **kw)
        return ei.value.status

    s0 = torch.cuda.current_stream().cuda_stream
    assert status(s0, dt=F32) == UNSUPPORTED and status(s0, D_=48) == UNSUPPORTED
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        refused = status(side.cuda_stream)
    assert refused == bsmr.NOT_PREPARED and not plan.attention_panels_prepared(D, Dv)
    torch.cuda.synchronize()
    assert (bufO.cpu().numpy().view(np.uint32) == FILL_BITS).all() and (bufL.cpu().numpy().view(np.uint32) == FILL_BITS).all()
    plan.prepare_attention_panels(D, Dv)
    assert plan.attention_panels_prepared(D, Dv) and plan.attention_stats()["segments"] == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # the first launch of the plan is the captured one
        launch(side.cuda_stream)
    eager = once(plan_of(name), Q, K, V, 0.125, F16)  # a lazily built plan
    for _ in range(3):
        dO.fill_(float("nan"))
        dL.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        AC.check_exact(dO.cpu().numpy().reshape(plan.M, Dv), eager[0], "replay O")
        AC.check_exact(dL.cpu().numpy(), eager[1], "replay LSE")


def test_autograd_against_dense_float64_attention():
    # tolerance: 8 x the error of the same dense attention computed in float16 on the CPU, against float64
    torch = torch_cuda()
    from bsmr import autograd
    from test_gpu_attention_fused_autograd import _dense_attention, _t
    pat = AC.pattern("zipf_shuffled")
    plan = AC.make_plan(pat)
    M, N, D = pat[0], pat[1], 64
    Q, K, V, dO = (half_values(AC.signed_data(r * D, 81 + i).reshape(r, D), F16) for i, r in enumerate((M, N, N, M)))
    ref = _dense_attention(pat, Q, K, V, dO, D ** -0.5, np.float64)
    cpu = _dense_attention(pat, Q, K, V, dO, D ** -0.5, np.float16)
    tQ, tK, tV = (_t(torch, X, torch.float16) for X in (Q, K, V))
    O = autograd.attention_fused(plan, tQ, tK, tV, forward="panels", backward="fused")
    O.backward(torch.from_numpy(dO).cuda())
    torch.cuda.synchronize()
    assert plan.attention_panels_stats()["items"] > 0 and plan.attention_stats()["segments"] == 0
    for what, g, r, c in zip(("O", "dQ", "dK", "dV"), (O.detach(), tQ.grad, tK.grad, tV.grad), ref, cpu):
        top = np.abs(r).max()
        cpu_err = np.abs(c.astype(np.float64) - r).max() / top
        gpu_err = np.abs(g.float().cpu().numpy().astype(np.float64) - r).max() / top
        print(f"ATTENTION_PANELS_AUTOGRAD f16 {what}: float16 CPU error {cpu_err:.3e}, GPU error {gpu_err:.3e}")
        assert 0 < cpu_err and gpu_err <= 8 * cpu_err, what
