"""GPU: one long-lived plan driven through every operation in mixed order (tests/lifetime_cases.py).

Per sequence and plan there is the long-lived plan L and, per family, a fresh projection plan that
receives only that family's steps and the recolumn calls. Held, with no tolerance anywhere:

  * non-interference: every output of every step on L equals the projection plan's bit for bit
    (NaN payloads included), on both data sets;
  * anchor: on the exact data sets L also equals the float64 reference of the step's cases module,
    by that module's own exact assertion (two plans wrong in the same way would agree);
  * host-visible state after every step: every *_prepared query and every stats call of L equals
    the model's prediction (lifetime_cases.Model, a restatement of include/bsmr.h), and the stats of
    the state a step touched equal the projection plan's;
  * after a recolumn, check(K, dtype) passes for every (K, dtype) launched since;
  * a refused call raises the status of its family's edge test and leaves its NaN outputs NaN;
  * no other step raises: nothing is skipped or answered UNSUPPORTED;
  * at the end a plan of sddmm_cases.ONE_PER_KIND shows its case's launch-path evidence.

Modes: `synced` synchronises after every step; `back_to_back` gives every step its own NaN-filled
outputs on the current stream and synchronises once, at the end, so that lazy builds, scratch grows
and recolumn happen while earlier launches are still queued (the projection plans run synced).
No graph capture: growing or rebuilding state frees what an earlier capture points at.
"""
import functools

import numpy as np
import pytest

import attention_bwd_cases as BC
import attention_cases as AC
import attention_heads_cases as HC
import bsmr
import lifetime_cases as LC
import sddmm_cases as DC
import softmax_cases as SC
import spmm_cases as PC
from bsmr import BF16, F16, F32, Plan
from gpu_util import path_evidence, plan_launch, to_device, torch_cuda
from lifetime_cases import arg

pytestmark = pytest.mark.gpu

DEFAULT_PLANS = {"default_hub": ("hub", 128, BF16), "default_hub_T": ("hub_T", 64, F32),
                 "default_zipf_shuffled": ("zipf_shuffled", 64, F16)}
PLANS = list(DC.ONE_PER_KIND) + list(DEFAULT_PLANS)
SEQUENCES = LC.hand_written()
SCALE = 0.125          # a power of two: the exact sets stay exact
SCALE_SOFTMAX_BWD = 0.5
STATS_FIELDS = ("num_row_panels", "num_dense_tiles", "num_residual", "dense_items", "residual_items", "rb_rows",
                "rb_items", "rb_pieces", "rb_entries", "rb_tiles", "rb_work_items", "dense_sampled_tiles",
                "rb_orig_rows", "ptile_items", "rb_pairs", "rb_batches", "rb_col_blocks")
TOUCHES = {"spmm": ("spmm1", "spmm2"), "softmax": ("softmax",), "attn": ("attn",), "attn_bwd": ("bwd",)}


# ------------------------------------------------------------------- plans and facts ----
@functools.lru_cache(maxsize=None)
def pattern(name):
    try:
        return DC.pattern(name)
    except KeyError:
        return BC.pattern(name)


def spec(name):
    """(pattern name, K, dtype, Plan keyword arguments, the sddmm_cases case or None)."""
    if name in DEFAULT_PLANS:
        pn, K, dt = DEFAULT_PLANS[name]
        return pn, K, dt, dict(alpha=0.3, delta=0.3, free_mem_bytes=DC.FREE), None
    case = DC.BY_NAME[name]
    return case.pattern, case.K, case.dtype, DC.plan_kwargs(case), case


def make_plan(name, delta=0.3):
    pn, _, _, kw, _ = spec(name)
    M, N, rp, ci = pattern(pn)
    return Plan(M, N, rp, ci, **dict(kw, delta=delta))


@functools.lru_cache(maxsize=None)
def facts_of(name):
    """(lifetime_cases.Facts, reorderedRows): the launch kind and row-block slot per (delta, K, dtype)
    as the library decides them on a throw-away plan built at that delta."""
    pn, K, dt, _, _ = spec(name)
    launch, P, rows = {}, 0, None
    for delta in LC.DELTAS:
        probe = make_plan(name, delta)
        for d, k, t in LC.launch_keys(K, dt):
            if d == delta:
                la = plan_launch(probe, k, t)
                launch[(d, k, t)] = (la["kind"], la["slot"])
        if delta == 0.3:
            P, rows = probe.stats()["num_row_panels"], probe.array("reorderedRows")
    return LC.Facts(name, pattern(pn), K, dt, P, launch), rows


# ------------------------------------------------------------------------- host data ----
@functools.lru_cache(maxsize=None)
def sddmm_data(pn, K, dt, data, seed):
    pat = pattern(pn)
    gen = DC.grid_data if data == "exact" else DC.signed_data
    A = DC.as_seen(gen(pat[0] * K, 101 + 2 * seed), dt).reshape(pat[0], K)
    B = DC.as_seen(gen(pat[1] * K, 202 + 2 * seed), dt).reshape(pat[1], K)
    return A, B, (DC.sddmm_ref(pat, A, B)[0] if data == "exact" else None)


@functools.lru_cache(maxsize=None)
def spmm_data(pn, side, K, dt, data):
    pat = pattern(pn)
    n = pat[1] if side == 1 else pat[0]
    exact = data == "exact"
    V = (PC.grid_values if exact else PC.signed_values)(len(pat[3]), 31)
    X = DC.as_seen((DC.grid_data if exact else DC.signed_data)(n * K, 32 + side), dt).reshape(n, K)
    return V, X, (PC.spmm_ref(pat, side, V, X) if exact else None)


@functools.lru_cache(maxsize=None)
def softmax_data(pn, op, data):
    """(inputs, scale, the exact answer or None)."""
    pat = pattern(pn)
    if op == "softmax":
        if data == "exact":
            P, W = SC.one_hot(pat)
            return (P,), SCALE, W
        return (SC.signed_scores(pat, "wide", 41),), SCALE, None
    if data == "exact":
        W, G = SC.backward_grid(pat, 43)
        ref = SC.backward_ref(pat, W, G, SCALE_SOFTMAX_BWD)["dP"]
        want = ref.astype(np.float32)
        assert (want.astype(np.float64) == ref).all()
        return (W, G), SCALE_SOFTMAX_BWD, want
    return SC.backward_signed(pat, SCALE, 45), SCALE, None


@functools.lru_cache(maxsize=None)
def attn_data(pn, cfg, data, seed=5):
    pat = pattern(pn)
    D, Dv, dt = LC.SHAPES[cfg]
    if data == "exact":
        Q, K, V, winner, pi, base = AC.selector(pat, D, Dv, "random", dt, seed)
        O, LSE = AC.selector_expected(V, winner, pi, base, SCALE, dt)
        return dict(Q=Q, K=K, V=V, O=O, LSE=LSE)
    Q, K, V, _ = AC.signed_inputs(pat, D, Dv, "wide", SCALE, seed)
    return dict(Q=Q, K=K, V=V)


@functools.lru_cache(maxsize=None)
def bwd_data(pn, cfg, data, seed=17):
    pat = pattern(pn)
    D, Dv, dt = LC.SHAPES[cfg]
    if data == "exact":
        x = BC.flat_inputs(pat, D, Dv, dt, seed)
        return dict(zip(("Q", "K", "V", "O", "GO", "LSE"), x), ref=BC.backward_ref(pat, *x, SCALE, dt))
    return dict(zip(("Q", "K", "V", "O", "GO", "LSE"), BC.signed_inputs(pat, D, Dv, "wide", SCALE, dt, seed)[:6]))


def slice_seeds(bh):
    B, H = LC.HEADS_BH[bh]
    return [HC.SEED0 + HC.SEED_STEP * z for z in range(B * H)]


# ----------------------------------------------------------------------- device data ----
DEV = {}


def dev(key, make):
    """A read-only device input, uploaded once per process."""
    if key not in DEV:
        DEV[key] = make()
    return DEV[key]


def nan(*shape):
    torch = torch_cuda()
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def stream():
    return torch_cuda().cuda.current_stream().cuda_stream


def heads_input(pn, cfg, data, bh, which, key, dt):
    """(Z, rows, W) slices as a (B, H, rows, W) device view of a dense (B, rows, H, W) tensor (with
    one head the two layouts coincide: a dimension of extent 1 is never stepped over)."""
    B, H = LC.HEADS_BH[bh]
    src = attn_data if which == "fwd" else bwd_data

    def place():
        X = np.stack([src(pn, cfg, data, s)[key] for s in slice_seeds(bh)])
        t = to_device(X.reshape((B, H) + X.shape[1:]), dt)
        return t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)

    return dev(("heads", pn, cfg, data, bh, which, key), place)


def heads_output(B, H, rows, W):
    """A NaN-filled (B, rows, H, W) buffer seen as (B, H, rows, W): the bmhd layout."""
    return nan(B, rows, H, W).permute(0, 2, 1, 3)


# ------------------------------------------------------------------ one step on a plan ----
class Refused(Exception):
    pass


def run_step(plan, pn, rows, c):
    """Launch the concrete step `c`: (outputs {name: device tensor}, host result or None). No
    synchronisation but what the call itself does."""
    torch = torch_cuda()
    pat = pattern(pn)
    M, N, _, ci = pat
    nnz = len(ci)
    a, op, s = dict(c.args), c.op, stream()
    if op == "refused":
        return run_refused(plan, pn, c)
    if op == "recolumn":
        plan.recolumn(a["delta"])
        return {}, None
    if c.family in ("sddmm", "panels"):
        K, dt = a["K"], a["dtype"]
        if op == "prepare":
            plan.prepare(K, dt)
            return {}, None
        if op == "check":
            return {}, plan.check(K, dt, verbose=False)
        if op == "stats":
            st = plan.stats()
            return {}, {k: st[k] for k in STATS_FIELDS}
        if op == "prepare_panels":
            plan.prepare(K, dt, panels=a["ranges"][0], local=a["local"])
            return {}, None
        nb = 3 if op == "sddmm_batch" else 1
        ops = [sddmm_data(pn, K, dt, a["data"], b) for b in range(nb)]
        dA = dev(("A", pn, K, dt, a["data"], nb), lambda: to_device(np.stack([o[0] for o in ops]), dt))
        dB = dev(("B", pn, K, dt, a["data"], nb), lambda: to_device(np.stack([o[1] for o in ops]), dt))
        P = nan(nb * nnz)
        if op == "sddmm":
            plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, P.data_ptr(), stream=s, dtype=dt)
        elif op == "sddmm_batch":
            plan.sddmm_batch(nb, dA.data_ptr(), dB.data_ptr(), K, P.data_ptr(), stream=s, dtype=dt)
        else:
            for p0, p1 in a["ranges"]:
                if op == "panels_local":
                    dL = dev(("Aloc", pn, K, dt, a["data"], p0, p1),
                             lambda: to_device(ops[0][0][rows[16 * p0:16 * p1]], dt))
                    plan.sddmm_panels_local(dL.data_ptr(), dB.data_ptr(), K, P.data_ptr(), p0, p1, stream=s, dtype=dt)
                else:
                    plan.sddmm_panels(dA.data_ptr(), dB.data_ptr(), K, P.data_ptr(), p0, p1, stream=s, dtype=dt)
        return {"P": P}, None
    if c.family == "spmm":
        K, dt = a["K"], a["dtype"]
        if op == "prepare_spmm":
            plan.prepare_spmm(K, a["sides"], a["chunk"])
            return {}, None
        out = {}
        sides = {"spmm": (1,), "spmm_t": (2,), "sddmm_backward": (1, 2)}[op]
        dV = dev(("V", pn, a["data"]), lambda: torch.from_numpy(spmm_data(pn, 1, K, dt, a["data"])[0]).cuda())
        dX = {sd: dev(("X", pn, sd, K, dt, a["data"]), lambda: to_device(spmm_data(pn, sd, K, dt, a["data"])[1], dt))
              for sd in (1, 2)}
        for sd in sides:
            out["GA" if sd == 1 else "GB"] = nan(M if sd == 1 else N, K)
        if op == "sddmm_backward":  # dA is spmm_t's operand, dB spmm's
            plan.sddmm_backward(dV.data_ptr(), dX[2].data_ptr(), dX[1].data_ptr(), K, out["GA"].data_ptr(),
                                out["GB"].data_ptr(), stream=s, dtype=dt)
        elif op == "spmm":
            plan.spmm(dV.data_ptr(), dX[1].data_ptr(), K, out["GA"].data_ptr(), stream=s, dtype=dt)
        else:
            plan.spmm_t(dV.data_ptr(), dX[2].data_ptr(), K, out["GB"].data_ptr(), stream=s, dtype=dt)
        return out, None
    if c.family == "softmax":
        if op == "prepare_softmax":
            plan.prepare_softmax()
            return {}, None
        xs, scale, _ = softmax_data(pn, op, a["data"])
        d = [dev(("sm", pn, op, a["data"], i), lambda: SC.dev(x)) for i, x in enumerate(xs)]
        W = nan(nnz)
        if op == "softmax":
            plan.softmax(d[0].data_ptr(), W.data_ptr(), scale, stream=s)
        else:
            plan.softmax_backward(d[0].data_ptr(), d[1].data_ptr(), W.data_ptr(), scale, stream=s)
        return {"W": W}, None
    D, Dv, dt, cfg = a["D"], a["Dv"], a["dtype"], a["cfg"]
    if op == "prepare_attention":
        plan.prepare_attention(D, Dv)
        return {}, None
    if op == "prepare_attention_backward":
        plan.prepare_attention_backward(D, Dv)
        return {}, None
    if op == "attention":
        x = attn_data(pn, cfg, a["data"])
        q, k, v = (dev(("attn", pn, cfg, a["data"], n), lambda: to_device(x[n], dt)) for n in "QKV")
        out = {"O": nan(M, Dv)}
        if a["lse"]:
            out["LSE"] = nan(M)
        plan.attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), D, Dv, out["O"].data_ptr(),
                       out["LSE"].data_ptr() if a["lse"] else 0, SCALE, stream=s, dtype=dt)
        return out, None
    shapes = dict(GQ=(M, D), GK=(N, D), GV=(N, Dv))
    if op == "attention_backward":
        x = bwd_data(pn, cfg, a["data"])
        d = [dev(("bwd", pn, cfg, a["data"], n), lambda: to_device(x[n], dt if n in "QKV" else F32))
             for n in ("Q", "K", "V", "O", "GO", "LSE")]
        out = {n: nan(*shapes[n]) for n in a["want"]}
        ptr = {n: (out[n].data_ptr() if n in out else 0) for n in shapes}
        plan.attention_backward(*(t.data_ptr() for t in d), D, Dv, ptr["GQ"], ptr["GK"], ptr["GV"], SCALE, stream=s,
                                dtype=dt)
        return out, None
    B, H = LC.HEADS_BH[a["bh"]]
    if op == "attention_heads":
        q, k, v = (heads_input(pn, cfg, a["data"], a["bh"], "fwd", n, dt) for n in "QKV")
        out = {"O": heads_output(B, H, M, Dv), "LSE": nan(B, H, M)}
        plan.attention_heads(B, H, q, k, v, D, Dv, out["O"], out["LSE"].data_ptr(), SCALE, stream=s, dtype=dt)
        return out, None
    assert op == "attention_backward_heads", op
    d = [heads_input(pn, cfg, a["data"], a["bh"], "bwd", n, dt if n in "QKV" else F32)
         for n in ("Q", "K", "V", "O", "GO")]
    lse = dev(("heads", pn, cfg, a["data"], a["bh"], "lse"), lambda: to_device(
        np.stack([bwd_data(pn, cfg, a["data"], sd)["LSE"] for sd in slice_seeds(a["bh"])]).reshape(B, H, M), F32))
    out = {n: heads_output(B, H, *shapes[n]) for n in a["want"]}
    plan.attention_backward_heads(B, H, *d, lse.data_ptr(), D, Dv, out.get("GQ"), out.get("GK"), out.get("GV"), SCALE,
                                  stream=s, dtype=dt)
    return out, None


def run_refused(plan, pn, c):
    """A call the library must refuse: ({its NaN outputs}, the status it raised)."""
    torch = torch_cuda()
    M, N, _, ci = pattern(pn)
    nnz, what, s = len(ci), arg(c, "what"), stream()
    junk = dev(("junk", pn), lambda: torch.zeros(max(M, N, 16) * 128 + 64, dtype=torch.float32, device="cuda"))
    j = junk.data_ptr()
    q = j + 4 if what == "misaligned" else j
    D = 24 if what == "bad_d" else 32
    scale = 0.0 if what == "scale0" else 1.0
    shared = lambda p, W: (p, 0, 0, W)  # noqa: E731  (one operand shared by every slice is a legal input)
    ptr = lambda t: t.data_ptr()  # noqa: E731
    if c.family == "sddmm":
        out = {"P": nan(nnz)}
        fn, args = plan.sddmm, (j, j, 24, ptr(out["P"]))
    elif c.family == "panels":
        out = {"P": nan(nnz)}
        fn, args = plan.sddmm_panels, (j, j, 24, ptr(out["P"]), 0, 1)
    elif c.family == "spmm":
        out = {"Y": nan(M, 32)}
        fn, args = plan.spmm, (j, j, 24, ptr(out["Y"]))
    elif c.family == "softmax":
        out = {"W": nan(nnz)}
        fn, args = plan.softmax, (j, ptr(out["W"]), scale)
    elif c.family == "attn":
        out = {"O": nan(M, 48), "LSE": nan(M)}
        fn, args = plan.attention, (q, j, j, D, 48, ptr(out["O"]), ptr(out["LSE"]), scale)
    elif c.family == "attn_bwd":
        out = dict(GQ=nan(M, 32), GK=nan(N, 32), GV=nan(N, 48))
        g = [0 if what == "all_null" else ptr(out[n]) for n in BC.OUTPUTS]
        fn, args = plan.attention_backward, (q, j, j, j, j, j, D, 48, g[0], g[1], g[2], scale)
    elif what == "all_null":
        out = {}
        fn = plan.attention_backward_heads
        args = (1, 3, shared(j, 32), shared(j, 32), shared(j, 48), shared(j, 48), shared(j, 48), j, 32, 48, None, None,
                None, 1.0)
    else:
        out = {"O": nan(1, 3, M, 48), "LSE": nan(1, 3, M)}
        fn = plan.attention_heads
        args = (1, 3, shared(q, 32), shared(j, 32), shared(j, 48), D, 48, out["O"], ptr(out["LSE"]), scale)
    with pytest.raises(bsmr.BsmrError) as ei:
        fn(*args, stream=s)
    return out, ei.value.status


def to_host(outs):
    return {k: np.ascontiguousarray(t.cpu().numpy()) for k, t in outs.items()}


# -------------------------------------------------------------------------- observers ----
def ask(plan, key):
    kind = key[0]
    if kind == "sddmm":
        return plan.prepared(key[1], key[2])
    if kind == "panels":
        return plan.prepared(key[1], key[2], panels=(key[3], key[4]), local=key[5])
    if kind == "spmm":
        return plan.spmm_prepared(key[1], key[2])
    if kind == "softmax":
        return plan.softmax_prepared()
    fn = plan.attention_heads_prepared if kind == "attn" else plan.attention_backward_heads_prepared
    one = plan.attention_prepared if kind == "attn" else plan.attention_backward_prepared
    got = fn(key[1], key[2], key[3])
    assert key[3] != 1 or got == one(key[1], key[2]), f"{key}: the single-slice query disagrees with slices = 1"
    return got


def all_stats(plan):
    return dict(spmm1=plan.spmm_stats(1), spmm2=plan.spmm_stats(2), softmax=plan.softmax_stats(),
                attn=plan.attention_stats(), bwd=plan.attention_backward_stats())


def hold_to_model(plan, model, what):
    """Every *_prepared query and every stats call against the model; returns the stats."""
    want = model.prepared()
    got = {k: ask(plan, k) for k in want}
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, f"{what}: *_prepared (library, model) differ at {bad}"
    st, ws = all_stats(plan), model.stats()
    bad = {k: (st[k], ws[k]) for k in ws if st[k] != ws[k]}
    assert not bad, f"{what}: stats (library, model) differ at {bad}"
    return st


def touched(c):
    """The stats a step's call may change (a refused call and recolumn: none)."""
    if c.op == "refused":
        return ()
    if c.family == "heads":
        return ("attn",) if c.op == "attention_heads" else ("bwd",)
    return TOUCHES.get(c.family, ())


# ---------------------------------------------------------------------------- anchors ----
def written_by(rows, pat, ranges):
    M, _, rp, _ = pat
    mine = np.zeros(M, bool)
    for p0, p1 in ranges:
        mine[rows[16 * p0:16 * p1]] = True
    return mine[PC.entry_rows(M, rp)]


def anchor(pn, rows, c, out, what):
    """On the exact data sets the step's outputs equal the float64 reference of its cases module."""
    pat = pattern(pn)
    a, op = dict(c.args), c.op
    if a.get("data") != "exact":
        return
    if c.family in ("sddmm", "panels"):
        nnz = len(pat[3])
        P = out["P"].reshape(-1, nnz)
        for b in range(len(P)):
            ref = sddmm_data(pn, a["K"], a["dtype"], "exact", b)[2]
            mask = written_by(rows, pat, a["ranges"]) if "ranges" in a else np.ones(nnz, bool)
            assert np.isnan(P[b][~mask]).all(), f"{what}: entries outside the panel ranges were written"
            DC.assert_exact(P[b][mask], ref[mask], what)
    elif c.family == "spmm":
        for name, side in (("GA", 1), ("GB", 2)):
            if name in out:
                PC.assert_exact(out[name], spmm_data(pn, side, a["K"], a["dtype"], "exact")[2], f"{what} {name}")
    elif c.family == "softmax":
        SC.check_exact(out["W"], softmax_data(pn, op, "exact")[2], pat, what)
    elif op == "attention":
        x = attn_data(pn, a["cfg"], "exact")
        AC.check_exact(out["O"], x["O"], f"{what} O")
        if "LSE" in out:
            AC.check_exact(out["LSE"], x["LSE"], f"{what} LSE")
    elif op == "attention_backward":
        BC.check_exact_all({n: out.get(n) for n in BC.OUTPUTS}, bwd_data(pn, a["cfg"], "exact")["ref"], what)
    elif op == "attention_heads":
        B, H = LC.HEADS_BH[a["bh"]]
        for z, sd in enumerate(slice_seeds(a["bh"])):
            x = attn_data(pn, a["cfg"], "exact", sd)
            AC.check_exact(out["O"][z // H, z % H], x["O"], f"{what} O slice {z}")
            AC.check_exact(out["LSE"][z // H, z % H], x["LSE"], f"{what} LSE slice {z}")
    else:
        B, H = LC.HEADS_BH[a["bh"]]
        for z, sd in enumerate(slice_seeds(a["bh"])):
            got = {n: (out[n][z // H, z % H] if n in out else None) for n in BC.OUTPUTS}
            BC.check_exact_all(got, bwd_data(pn, a["cfg"], "exact", sd)["ref"], f"{what} slice {z}")


# ------------------------------------------------------------------------- a sequence ----
def run_plan(name, plan, steps, synced, hold=True):
    """Drive `plan` through the abstract steps: [(concrete step, outputs on the host, host result,
    stats after the step)]. With `hold` the model is held after every step, check() after every
    recolumn, and a refused call to its status and untouched outputs."""
    torch = torch_cuda()
    facts, rows = facts_of(name)
    pn = spec(name)[0]
    model = LC.Model(facts)
    log, since, recolumned = [], [], False
    for i, step in enumerate(steps):
        c = LC.concrete(step, facts, model.delta)
        outs, host = run_step(plan, pn, rows, c)
        model.apply(c)
        if synced:
            torch.cuda.synchronize()
        what = f"{name} step {i} {c.op} {dict(c.args)}"
        st = hold_to_model(plan, model, what) if hold else all_stats(plan)
        if c.op == "recolumn":
            since, recolumned = [], True
        elif c.family == "sddmm" and c.op in LC.LAUNCHES:
            kd = (arg(c, "K"), arg(c, "dtype"))
            if kd not in since:
                since.append(kd)
                if hold and synced and recolumned:
                    assert plan.check(*kd, verbose=False) == (True, ""), f"{what}: check() after recolumn"
        log.append([c, outs, host, st])
    torch.cuda.synchronize()
    if hold and recolumned:
        for kd in since:
            assert plan.check(*kd, verbose=False) == (True, ""), f"{name}: check{kd} after the last recolumn"
    for entry in log:
        entry[1] = to_host(entry[1])
    if hold:
        for i, (c, outs, host, _) in enumerate(log):
            what = f"{name} step {i} {c.op} {dict(c.args)}"
            if c.op == "refused":
                assert host == LC.REFUSED[c.family][arg(c, "what")], f"{what}: status {host}"
                assert all(np.isnan(v).all() for v in outs.values()), f"{what}: a refused call wrote an output"
            elif c.op == "check":
                assert host == (True, ""), f"{what}: {host}"
            anchor(pn, rows, c, outs, what)
    return log


@functools.lru_cache(maxsize=2)  # (the two modes of one sequence follow each other)
def projections(name, key):
    """Per family the log of a fresh plan that receives only that family's steps and the recolumn
    calls, synchronised after every step: {family: {index in the sequence: log entry}}."""
    steps = sequence(key)
    out = {}
    for f in LC.FAMILIES:
        idx = [i for i, s in enumerate(steps) if s.family == f or s.op == "recolumn"]
        if any(steps[i].family == f for i in idx):
            out[f] = dict(zip(idx, run_plan(name, make_plan(name), [steps[i] for i in idx], True)))
    return out


def sequence(key):
    return SEQUENCES[key] if isinstance(key, str) else LC.random_sequence(key)


SUMMARY = {}


def run_case(name, key, mode):
    """The whole comparison of one (plan, sequence, mode); returns {stats at the end, the largest
    SpMM partial counts seen per side at chunk 32}."""
    if (name, key, mode) in SUMMARY:
        return SUMMARY[(name, key, mode)]
    steps = sequence(key)
    proj = projections(name, key)
    L = make_plan(name)
    log = run_plan(name, L, steps, mode == "synced")
    chunk32 = {1: 0, 2: 0}
    for i, (c, outs, host, st) in enumerate(log):
        what = f"{name} {key} {mode} step {i} {c.op} {dict(c.args)}"
        for side in (1, 2):
            if st[f"spmm{side}"]["chunk"] == 32:
                chunk32[side] = max(chunk32[side], st[f"spmm{side}"]["partials"])
        if c.op == "recolumn":
            continue
        pc, pouts, phost, pst = proj[c.family][i]
        assert pc == c
        assert set(pouts) == set(outs), what
        for k in outs:
            LC.assert_same_bits(outs[k], pouts[k], f"{what} {k}: the long-lived plan against the {c.family} plan")
        assert host == phost, f"{what}: host result {host} against the {c.family} plan's {phost}"
        for k in touched(c):
            drop = lambda d: {f: v for f, v in d.items() if not f.endswith("_bytes")}  # noqa: E731
            assert drop(st[k]) == drop(pst[k]), f"{what}: {k} stats {st[k]} against the {c.family} plan's {pst[k]}"
    assert len(log) == len(steps)  # (a step that raised, UNSUPPORTED included, never gets here)
    if key == "recolumn_between":  # without dense tiles every plan has a row-block slot: the local form ran
        assert any(c.op == "panels_local" and not arg(c, "substituted") for c, _, _, _ in log)
    case = spec(name)[4]
    if case is not None:
        assert not path_evidence(case, L)
    SUMMARY[(name, key, mode)] = dict(stats=log[-1][3], chunk32=chunk32)
    return SUMMARY[(name, key, mode)]


# ------------------------------------------------------------------------------ tests ----
@pytest.mark.parametrize("mode", ["synced", "back_to_back"])
@pytest.mark.parametrize("key", sorted(SEQUENCES))
@pytest.mark.parametrize("name", PLANS)
def test_hand_written_sequence(name, key, mode):
    run_case(name, key, mode)


@pytest.mark.parametrize("seed", LC.RANDOM_SEEDS)
@pytest.mark.parametrize("name", PLANS)
def test_random_sequence_back_to_back(name, seed):
    run_case(name, seed, "back_to_back")


@pytest.mark.parametrize("name", PLANS)
def test_imported_plan(name):
    """Plan.from_row_stage(*export_rows()) is a second way into all of it: one exact and one signed
    step of every family, bit-equal to the plan that Plan(...) built."""
    pn, _, _, kw, _ = spec(name)
    _, _, rp, ci = pattern(pn)
    made = make_plan(name)
    hdr, rws = made.export_rows()
    imported = Plan.from_row_stage(rp, ci, hdr, rws, delta=0.3, layout=kw.get("layout", "auto"),
                                   tuning=kw.get("tuning"))
    steps = [LC.use(f, data, cfg) for f in LC.FAMILIES for data, cfg in (("exact", 0), ("signed", 1))]
    steps += [LC.st("panels", "panels_local", data="exact"), LC.st("sddmm", "sddmm_batch", data="exact"),
              LC.st("heads", "attention_backward_heads", cfg=1, data="exact", bh=1, want=LC.SUBSETS[0])]
    a = run_plan(name, made, steps, True)
    b = run_plan(name, imported, steps, True)
    for i, ((c, oa, _, sa), (_, ob, _, sb)) in enumerate(zip(a, b)):
        assert set(oa) == set(ob)
        for k in oa:
            LC.assert_same_bits(ob[k], oa[k], f"{name} step {i} {c.op} {k}: the imported plan against Plan(...)")
        assert sa == sb
    for k in STATS_FIELDS:
        assert imported.stats()[k] == made.stats()[k], k


def test_every_split_path_ran():
    """From the stats, not from copied constants: across the default-option plans the sequences ran
    the split rows of the forward, the split rows and columns of the backward and, at chunk 32,
    partial rows on both SpMM sides."""
    runs = [run_case(name, "first_use_forward", "synced") for name in DEFAULT_PLANS]
    assert any(r["stats"]["attn"]["split_rows"] > 0 for r in runs)
    assert any(r["stats"]["bwd"]["row_split"] > 0 for r in runs)
    assert any(r["stats"]["bwd"]["col_split"] > 0 for r in runs)
    for side in (1, 2):
        assert any(r["chunk32"][side] > 0 for r in runs), f"no SpMM partial row on side {side} at chunk 32"
