"""GPU: the panel form of the fused attention backward on matrix instructions
(bsmr_attention_backward_panels), fp16 / bf16 at (D, Dv) forms that cover every
value of either, on the smallest patterns that can break it, each with its transpose so that the
columns side sees what the rows side sees.

Exact sets (section 14): flat_inputs as it is, and the selector with V on the k / 8 grid in place of
its uniform V (O = V[winner] follows it): this path computes g on the MFMA and delta on the vector ALU,
in different orders, so g - delta is exactly 0 only where dot(GO, V) is exact in every order: products
on the 1 / 64 grid, at most 16 each, 128 of them. On both sets GO, w in {0, 1} and dp (at most 7
significant bits) survive the rounding to fp16 and bf16 unchanged, which test 1 checks on the CPU first.

Bound on signed data: attention_bwd_cases.backward_bound plus panel_bwd_terms (derived in section 19).
"""
import functools

import numpy as np
import pytest

import attention_bwd_cases as ABC
import attention_cases as AC
import bsmr
from attention_bwd_cases import OUTPUTS, _dst_sums
from attention_cases import FILL_BITS, filled
from bsmr import BF16, F16, F32
from gpu_util import half_values, torch_cuda
from sddmm_cases import grid_data
from test_gpu_attention_panels import pattern as base_pattern

pytestmark = pytest.mark.gpu
UNSUPPORTED = 6
FORMS = [pytest.param(dt, D, Dv, id=f"{AC.DTYPE_NAME[dt]}-{D}-{Dv}") for dt in (F16, BF16)
         for D, Dv in [(32, 32), (64, 128), (128, 64)]]
BASE = ["staircase37", "union_32_33", "empty_row_and_panel", "split", "hub"]
PATTERNS = BASE + [n + "_T" for n in BASE]


@functools.lru_cache(maxsize=None)
def pattern(name):
    return ABC.transpose(base_pattern(name[:-2])) if name.endswith("_T") else base_pattern(name)


@functools.lru_cache(maxsize=None)
def plan_of(name):
    return AC.make_plan(pattern(name))


def lists_of(name):
    """(rows side, columns side) host lists: over the plan's own row order, and of the transpose."""
    M, N, rp, ci = pattern(name)
    return (bsmr.attention_panel_lists(M, N, rp, ci, plan_of(name).array("reorderedRows")),
            bsmr.attention_panel_lists(*bsmr.attention_pattern_transpose(M, N, rp, ci)))


def once(plan, dev, D, Dv, scale, dtype, want=OUTPUTS, fn="attention_backward_panels"):
    """dict(GQ, GK, GV) of one launch on device operands (None for an output not in `want`). Every
    output starts as FILL_BITS with a guard zone behind it."""
    torch = torch_cuda()
    shapes = dict(GQ=(plan.M, D), GK=(plan.N, D), GV=(plan.N, Dv))
    bufs = {k: filled(r * c) for k, (r, c) in shapes.items()}
    ptr = [bufs[k][1].data_ptr() if k in want else 0 for k in OUTPUTS]
    getattr(plan, fn)(*(t.data_ptr() for t in dev), D, Dv, *ptr, scale, stream=torch.cuda.current_stream().cuda_stream,
                      dtype=dtype)
    torch.cuda.synchronize()
    out = {}
    for k, (r, c) in shapes.items():
        h = bufs[k][0].cpu().numpy()
        if k not in want:
            assert (h.view(np.uint32) == FILL_BITS).all(), f"{k} written though it was not asked for"
            out[k] = None
            continue
        assert (h[r * c:].view(np.uint32) == FILL_BITS).all(), f"a store past the end of {k}"
        assert not (h[:r * c].view(np.uint32) == FILL_BITS).any(), f"an element of {k} was never written"
        out[k] = h[:r * c].reshape(r, c)
    return out


def exact_sets(pat, D, Dv, dtype):
    """(what, (Q, K, V, O, GO, LSE), scale) of the exact sets (module docstring)."""
    for order, scale in (("random", 1.0), ("ascending", 0.125)):
        Q, K, _, winner, pi, base = AC.selector(pat, D, Dv, order, dtype)
        V = grid_data(pat[1] * Dv, 7).reshape(pat[1], Dv)
        O, LSE = AC.selector_expected(V, winner, pi, base, scale, dtype)
        yield f"selector {order}", (Q, K, V, O, grid_data(pat[0] * Dv, 8).reshape(pat[0], Dv), LSE), scale
    yield "flat", ABC.flat_inputs(pat, D, Dv, dtype), 0.5


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_exact_sets_are_bit_exact(dtype, D, Dv, name):
    pat, plan = pattern(name), plan_of(name)
    for what, ops, scale in exact_sets(pat, D, Dv, dtype):
        ref = ABC.backward_ref(pat, *ops, scale, dtype)
        for X in (ops[4], ref["w"], ref["dp"]):  # GO, w, dp: the rounding to the operand type changes nothing
            assert (half_values(X, dtype).astype(np.float64) == X).all(), what
        ABC.check_exact_all(once(plan, ABC.device_inputs(*ops, dtype), D, Dv, scale, dtype), ref, f"{name} {what}")
    st = plan.attention_backward_panels_stats()
    nnz = len(pat[3])
    for side, (_, cols, _, items, reds) in zip(("row", "col"), lists_of(name)):
        want = dict(panels=-(-pat[side == "col"] // 16), items=len(items), steps=len(cols), split_panels=len(reds),
                    partials=int(reds[:, 2].sum()) if len(reds) else 0,
                    fill_permille=1000 * nnz // (512 * len(cols)) if len(cols) else 0)
        assert {k: st[f"{side}_{k}"] for k in want} == want, side
    if name.startswith("split"):
        assert st["col_split_panels" if name.endswith("_T") else "row_split_panels"] >= 1
    assert st["delta_bytes"] >= 4 * pat[0] and st["row_scratch_bytes"] >= 64 * st["row_partials"] * D
    assert st["col_scratch_bytes"] >= 64 * st["col_partials"] * (D + Dv)


def panel_bwd_terms(ref, dtype):
    """dict(GQ, GK, GV): what this path adds per element to backward_bound (section 19), with
    u_T = 2^-11 (fp16) or 2^-8 (bf16): GO rounded once, |dg| <= u_T sum_k |GO V|, which reaches dp as
    scale w dg; dp rounded once, u_T sum |dp K| (GQ) and u_T sum |dp Q| (GK); w and GO rounded once
    each, (2 u_T + u_T^2) sum w |GO| (GV); fp16 only: 2^-25 absolute per rounded factor that can fall
    under 2^-14, times the largest other factor, per term."""
    uT, sub = (2.0 ** -11, 2.0 ** -25) if dtype == F16 else (2.0 ** -8, 0.0)
    rows, cols, M, N, w = ref["rows"], ref["cols"], ref["M"], ref["N"], ref["w"]
    aK, aQ, aGO = np.abs(ref["K"]), np.abs(ref["Q"]), np.abs(ref["GO"])
    dg = uT * ref["Sg"] + ref["Dv"] * sub * np.abs(ref["V"]).max()
    e = ref["scale"] * w * dg + uT * np.abs(ref["dp"])
    rl, cl = ref["rlen"].astype(np.float64)[:, None], ref["clen"].astype(np.float64)[:, None]
    return dict(GQ=_dst_sums(M, rows, e, aK, cols) + rl * sub * aK.max(initial=0),
                GK=_dst_sums(N, cols, e, aQ, rows) + cl * sub * aQ.max(initial=0),
                GV=(2 * uT + uT * uT) * _dst_sums(N, cols, w, aGO, rows) + cl * sub * (aGO.max(initial=0) + w.max(initial=0)))


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype,D,Dv", FORMS)
def test_against_float64(dtype, D, Dv, name):
    pat, plan = pattern(name), plan_of(name)
    for kind, scale in (("narrow", 1.0), ("wide", 1.0), ("narrow", D ** -0.5), ("wide", D ** -0.5)):
        Q, K, V, O, GO, LSE, opscale, _ = ABC.signed_inputs(pat, D, Dv, kind, scale, dtype)
        dev = ABC.device_inputs(Q, K, V, O, GO, LSE, dtype)
        got = once(plan, dev, D, Dv, scale, dtype)
        gather = once(plan, dev, D, Dv, scale, dtype, fn="attention_backward")
        ref = ABC.backward_ref(pat, Q, K, V, O, GO, LSE, scale, dtype)
        base, add = ABC.backward_bound(ref, opscale), panel_bwd_terms(ref, dtype)
        r = {}
        for k, lens in zip(OUTPUTS, (ref["rlen"], ref["clen"], ref["clen"])):
            Y = got[k].astype(np.float64)
            r[k] = AC._ratio(np.abs(Y - ref[k]), base[k] + add[k])
            r[k + "g"] = AC._ratio(np.abs(Y - gather[k]), 2 * base[k] + add[k])
            assert (got[k][lens == 0].view(np.uint32) == 0).all(), f"{k}: a destination without entries is not +0"
        print(f"RATIO attention_bwd_panels {AC.DTYPE_NAME[dtype]} {D} {Dv} {name} {kind} {scale:.4f}: " +
              " ".join(f"{k} {r[k]:.4f} vs gather {r[k + 'g']:.4f}" for k in OUTPUTS))
        assert max(r.values()) <= 1.0, (kind, scale, r)


def _signed_dev(name, D, Dv, dtype, scale=0.125):
    Q, K, V, O, GO, LSE, _, _ = ABC.signed_inputs(pattern(name), D, Dv, "narrow", scale, dtype)
    return (Q, K, V, O, GO, LSE), ABC.device_inputs(Q, K, V, O, GO, LSE, dtype)


@pytest.mark.parametrize("dtype,D,Dv,name", [(F16, 64, 128, "split"), (BF16, 32, 32, "split_T")])
def test_bitwise_properties(dtype, D, Dv, name):
    plan = AC.make_plan(pattern(name))  # a fresh plan, built lazily by its first launch
    _, dev = _signed_dev(name, D, Dv, dtype)
    full = once(plan, dev, D, Dv, 0.125, dtype)
    assert ABC.same_bits(full, once(plan, dev, D, Dv, 0.125, dtype)), "two launches differ"
    once(plan, dev, D, Dv, 0.125, dtype, fn="attention_backward")  # the gather backward in between
    assert ABC.same_bits(full, once(plan, dev, D, Dv, 0.125, dtype)), "a gather backward launch changed the result"
    prepared = AC.make_plan(pattern(name))
    prepared.prepare_attention_backward_panels(D, Dv)
    assert prepared.attention_backward_panels_prepared(D, Dv) and not prepared.attention_backward_prepared(D, Dv)
    assert ABC.same_bits(full, once(prepared, dev, D, Dv, 0.125, dtype)), "prepared and lazy plans differ"
    for want in (("GQ",), ("GK",), ("GV",), ("GQ", "GK"), ("GQ", "GV"), ("GK", "GV")):
        part = once(plan, dev, D, Dv, 0.125, dtype, want=want)
        assert all((part[k].view(np.uint32) == full[k].view(np.uint32)).all() for k in want), want
    with pytest.raises(bsmr.BsmrError):
        once(plan, dev, D, Dv, 0.125, dtype, want=())


@pytest.mark.parametrize("dtype,D,Dv,name", [(F16, 64, 128, "hub"), (BF16, 32, 32, "hub_T")])
def test_heads_slices_equal_the_single_slice_call(dtype, D, Dv, name):
    torch = torch_cuda()
    B, H = 2, 3  # (hub: split row panels; hub_T: split column panels: a scratch per slice)
    pat, plan = pattern(name), plan_of(name)
    M, N = pat[0], pat[1]
    tdt = torch.float16 if dtype == F16 else torch.bfloat16
    data = lambda n, seed, t=tdt: torch.from_numpy(AC.signed_data(n, seed)).to(t).cuda()  # noqa: E731
    Q = data(B * M * H * D, 1).view(B, M, H, D).transpose(1, 2)  # a view of a (B, M, H D) projection
    K = data(B * N * D, 2).view(B, 1, N, D).expand(B, H, N, D)   # one K / V for all heads: head stride 0
    V = data(B * N * Dv, 3).view(B, 1, N, Dv).expand(B, H, N, Dv)
    GO = data(B * H * M * Dv, 4, torch.float32).view(B, H, M, Dv)
    O, L = torch.empty(B, H, M, Dv, device="cuda"), torch.empty(B, H, M, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    plan.attention_panels_heads(B, H, Q, K, V, D, Dv, O, L.data_ptr(), 0.25, stream=s, dtype=dtype)
    GQ = torch.full((B, M, H, D), float("nan"), device="cuda").transpose(1, 2)
    GK, GV = torch.full((B, H, N, D), float("nan"), device="cuda"), torch.full((B, H, N, Dv), float("nan"), device="cuda")
    plan.attention_backward_panels_heads(B, H, Q, K, V, O, GO, L.data_ptr(), D, Dv, GQ, GK, GV, 0.25, stream=s, dtype=dtype)
    st = plan.attention_backward_panels_stats()
    assert st["col_partials" if name == "hub_T" else "row_partials"] >= 2
    for b in range(B):
        for h in range(H):
            q, k, v = (X[b, h].contiguous() for X in (Q, K, V))
            gq, gk, gv = (torch.empty(n, w, device="cuda") for n, w in ((M, D), (N, D), (N, Dv)))
            plan.attention_backward_panels(q.data_ptr(), k.data_ptr(), v.data_ptr(), O[b, h].data_ptr(), GO[b, h].data_ptr(),
                                           L[b, h].data_ptr(), D, Dv, gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), 0.25,
                                           stream=s, dtype=dtype)
            assert torch.equal(GQ[b, h], gq) and torch.equal(GK[b, h], gk) and torch.equal(GV[b, h], gv), (b, h)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_nan_stays_in_its_destinations_and_panels(dtype):
    name, D, Dv, i = "hub", 64, 64, 5
    pat, plan = pattern(name), plan_of(name)
    M, N, rp, ci = pat
    ops, dev = _signed_dev(name, D, Dv, dtype)
    clean = once(plan, dev, D, Dv, 0.125, dtype)
    (rows, rcols, _, ritems, _), (_, crows, _, citems, _) = lists_of(name)
    erows = AC.entry_rows(pat)
    j = int(ci[rp[i]])  # a column that a short row stores (the hub row stores it too)

    def sel(n, idx):
        m = np.zeros(n, bool)
        m[idx] = True
        return m

    storing, stored = sel(M, erows[ci == j]), sel(N, ci[rp[i]:rp[i + 1]])  # rows that store j; columns row i stores
    rpanel, cpanel = np.zeros(M, bool), np.zeros(N, bool)  # destinations of the panels whose union holds j / i
    for row0, step0, nsteps, _ in ritems:
        if (rcols[step0:step0 + nsteps] == j).any():
            rpanel[rows[row0:row0 + 16]] = True
    for col0, step0, nsteps, _ in citems:
        if (crows[step0:step0 + nsteps] == i).any():
            cpanel[col0:col0 + 16] = True
    assert not rpanel.all() and not cpanel.all(), "the pattern must have panels outside the sets"
    no_col, row_i, col_j = sel(N, []), sel(M, i), sel(N, j)
    # operand, index: (must, may) of GQ, GK, GV
    cases = {("Q", 0, i): ((row_i, row_i), (stored, cpanel), (stored, cpanel)),
             ("K", 1, j): ((storing, rpanel), (col_j, col_j), (col_j, col_j)),
             ("V", 2, j): ((storing, storing), (col_j, col_j), (no_col, no_col)),
             ("GO", 4, i): ((row_i, row_i), (stored, cpanel), (stored, cpanel)),
             ("LSE", 5, i): ((row_i, row_i), (stored, stored), (stored, stored))}
    for (what, x, idx), sets in cases.items():
        bad = [X.copy() for X in ops]
        bad[x][(idx, 3) if bad[x].ndim == 2 else idx] = np.nan
        got = once(plan, ABC.device_inputs(*bad, dtype), D, Dv, 0.125, dtype)
        for k, (must, may) in zip(OUTPUTS, sets):
            changed = (got[k].view(np.uint32) != clean[k].view(np.uint32)).any(axis=1)
            assert np.isnan(got[k][must]).any(axis=1).all() and not changed[~may].any(), (what, k)


def test_refused_shapes_and_capture():
    torch = torch_cuda()
    name, D, Dv, dtype = "split", 64, 32, F16
    plan = AC.make_plan(pattern(name))  # a fresh plan: nothing prepared
    _, dev = _signed_dev(name, D, Dv, dtype)
    bufs = [filled(n) for n in (plan.M * D, plan.N * D, plan.N * Dv)]

    def launch(s, D_=D, dt=dtype):
        plan.attention_backward_panels(*(t.data_ptr() for t in dev), D_, Dv, *(b[1].data_ptr() for b in bufs), 0.125,
                                       stream=s, dtype=dt)

    def status(s, **kw):
        with pytest.raises(bsmr.BsmrError) as ei:
            launch(s, **kw)
        return ei.value.status

    def untouched():
        torch.cuda.synchronize()
        return all((b[0].cpu().numpy().view(np.uint32) == FILL_BITS).all() for b in bufs)

    s0 = torch.cuda.current_stream().cuda_stream
    assert [status(s0, dt=F32), status(s0, D_=48), status(s0, D_=256)] == [UNSUPPORTED] * 3 and untouched()
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        refused = status(side.cuda_stream)
    assert refused == bsmr.NOT_PREPARED and not plan.attention_backward_panels_prepared(D, Dv) and untouched()
    plan.prepare_attention_backward_panels(D, Dv)
    assert plan.attention_backward_panels_prepared(D, Dv) and plan.attention_backward_stats()["col_segments"] == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # the first launch of the plan is the captured one
        launch(side.cuda_stream)
    eager = once(plan_of(name), dev, D, Dv, 0.125, dtype)  # another, lazily built plan
    for _ in range(3):
        for b in bufs:
            b[1].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k, b, (r, c) in zip(OUTPUTS, bufs, ((plan.M, D), (plan.N, D), (plan.N, Dv))):
            AC.check_exact(b[1].cpu().numpy().reshape(r, c), eager[k], f"replay {k}")


def test_autograd_against_dense_float64_attention():
    # tolerance: 8 x the error of the same dense attention computed in float16 on the CPU, against float64
    torch = torch_cuda()
    from bsmr import autograd
    from test_gpu_attention_fused_autograd import _dense_attention, _t
    pat = AC.pattern("zipf_shuffled")
    plan = AC.make_plan(pat)
    M, N, D = pat[0], pat[1], 64
    Q, K, V, dO = (half_values(AC.signed_data(r * D, 81 + n).reshape(r, D), F16) for n, r in enumerate((M, N, N, M)))
    ref = _dense_attention(pat, Q, K, V, dO, D ** -0.5, np.float64)
    cpu = _dense_attention(pat, Q, K, V, dO, D ** -0.5, np.float16)
    tQ, tK, tV = (_t(torch, X, torch.float16) for X in (Q, K, V))
    with pytest.raises(ValueError):
        autograd.attention_fused(plan, tQ.float(), tK.float(), tV.float(), backward="panels")
    O = autograd.attention_fused(plan, tQ, tK, tV, forward="panels", backward="panels")
    O.backward(torch.from_numpy(dO).cuda())
    torch.cuda.synchronize()
    assert plan.attention_backward_panels_stats()["col_items"] > 0 and plan.attention_backward_stats()["col_segments"] == 0
    for what, g, r, c in zip(("O", "dQ", "dK", "dV"), (O.detach(), tQ.grad, tK.grad, tV.grad), ref, cpu):
        top = np.abs(r).max()
        cpu_err = np.abs(c.astype(np.float64) - r).max() / top
        gpu_err = np.abs(g.float().cpu().numpy().astype(np.float64) - r).max() / top
        print(f"ATTENTION_BWD_PANELS_AUTOGRAD f16 {what}: float16 CPU error {cpu_err:.3e}, GPU error {gpu_err:.3e}")
        assert 0 < cpu_err and gpu_err <= 8 * cpu_err, what


def test_autograd_heads_equal_per_slice_calls():
    torch = torch_cuda()
    from bsmr import autograd
    name, H, D = "staircase37", 2, 32
    pat, plan = pattern(name), plan_of(name)
    Q, K, V, dO = (torch.from_numpy(AC.signed_data(H * r * D, 60 + n)).view(H, r, D).cuda()
                   for n, r in enumerate((pat[0], pat[1], pat[1], pat[0])))
    Q, K, V = (X.to(torch.bfloat16).requires_grad_(True) for X in (Q, K, V))
    autograd.attention_fused_heads(plan, Q, K, V, forward="panels", backward="panels").backward(dO)
    for h in range(H):
        q, k, v = (X[h].detach().clone().requires_grad_(True) for X in (Q, K, V))
        autograd.attention_fused(plan, q, k, v, forward="panels", backward="panels").backward(dO[h])
        assert all(torch.equal(X.grad[h], x.grad) for X, x in ((Q, q), (K, k), (V, v))), h
