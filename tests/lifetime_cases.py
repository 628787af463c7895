"""Sequences of operations on one long-lived plan, a host model of the state they leave, and the bit
comparison (no GPU here: tests/test_lifetime_cases_cpu.py checks this module,
tests/test_gpu_plan_lifetime.py runs it).

Every other GPU test builds a plan, uses one kernel family on it and throws it away. Here one plan
lives through a whole sequence in which every family is used in mixed order, and the test holds it
to a fresh plan per family that sees only that family's steps (and the recolumn calls). The family
split and the hand-written sequences follow the table of DESIGN.md section 17, "What a plan holds
and which call touches it": one sequence per way two calls can meet on a piece of state.

A step is Step(family, op, args), args a sorted tuple of (name, value) pairs:

  sddmm     sddmm, sddmm_batch (3 batches), prepare, check, stats            at the plan's (K, dtype)
  panels    panels, panels_local (the three uneven ranges of test_gpu_sddmm_float64, one output),
            prepare_panels (one range), panels_one (one of 17 distinct (K, range) layouts)
  spmm      spmm, spmm_t, sddmm_backward, prepare_spmm      kd: index into SPMM_KD (K 16 then 64)
  softmax   softmax, softmax_backward, prepare_softmax
  attn      attention (with and without LSE), prepare_attention          cfg: index into SHAPES
  attn_bwd  attention_backward (want: any non-empty subset of GQ / GK / GV), prepare_attention_backward
  heads     attention_heads, attention_backward_heads    bh: index into HEADS_BH, the bmhd layout
  plan      recolumn (delta in DELTAS)
  and, in any family, refused (what: a REFUSED kind): a call the library must turn down with the
  status of the family's edge test, writing nothing and changing nothing.

data: "exact" (sddmm_cases grid, spmm_cases grid, one-hot softmax, attention selector, backward
flat: the float64 answer bit for bit) or "signed". The steps are abstract: concrete() picks, per
plan and current delta, the (K, dtype) and panel ranges at which no call is answered UNSUPPORTED
(fp16 / bf16 panel ranges only where the plan has a row-block slot; the local form only where some
fp32 row size has one, else the plain panel launch stands in and the step says so: `substituted`;
at delta 1.1 no plan has a dense tile, so there every plan runs the local form).

Model: what the header promises about every *_prepared query and every stats call, as a function
of the steps so far and of a few facts about the plan (Facts: the pattern, the launch kind and
row-block slot per (delta, K, dtype), the panel count). It is a restatement of include/bsmr.h, not
of the code: layouts built on first use, dropped by recolumn or kept, two caches of sixteen panel
ranges, scratch that covers the largest need so far and never shrinks.
"""
import collections
import itertools

import numpy as np

import attention_bwd_cases as BC
import bsmr
import softmax_cases as SC
import spmm_cases as PC
from bsmr import F16, F32
from test_gpu_sddmm_float64 import _uneven_ranges as uneven_ranges

FAMILIES = ("sddmm", "panels", "spmm", "softmax", "attn", "attn_bwd", "heads")
SHAPES = [(32, 48, F32), (64, 64, F16)]  # (D, Dv, dtype): the generic lane form, a compile-time form
SPMM_KD = [(16, F32), (64, F16)]         # the scratch grows from the first to the second
PANEL_KD = [(32, F32), (64, F32)]        # row sizes of the 17 single-range layouts
DELTAS = (0.0, 0.3, 1.1)
HEADS_BH = [(1, 3), (2, 2), (1, 1)]
HEADS_LAYOUT = "bmhd"
SUBSETS = [w for n in (3, 2, 1) for w in itertools.combinations(("GQ", "GK", "GV"), n)]
CHUNKS = (0, 32, 0, PC.DEFAULT_CHUNK)    # bsmr_plan_prepare_spmm: keep, rebuild, keep, back to the default
N_CACHE_RANGES = 17                      # one more than either cache of panel ranges holds
MAX_RANGES = 16                          # include/bsmr.h: the 16 most recently prepared ranges
INVALID, UNSUPPORTED = 1, 6              # BSMR_ERR_INVALID, BSMR_ERR_UNSUPPORTED
REFUSED = {  # family -> {kind: status}, as the family's edge test expects it
    "sddmm": {"bad_k": UNSUPPORTED},
    "panels": {"bad_k": UNSUPPORTED},
    "spmm": {"bad_k": UNSUPPORTED},
    "softmax": {"scale0": INVALID},
    "attn": {"scale0": INVALID, "misaligned": INVALID, "bad_d": UNSUPPORTED},
    "attn_bwd": {"scale0": INVALID, "misaligned": INVALID, "bad_d": UNSUPPORTED, "all_null": INVALID},
    "heads": {"scale0": INVALID, "misaligned": INVALID, "bad_d": UNSUPPORTED, "all_null": INVALID},
}
OPS = {
    "sddmm": ("sddmm", "sddmm_batch", "prepare", "check", "stats"),
    "panels": ("panels", "panels_local", "prepare_panels", "panels_one"),
    "spmm": ("spmm", "spmm_t", "sddmm_backward", "prepare_spmm"),
    "softmax": ("softmax", "softmax_backward", "prepare_softmax"),
    "attn": ("attention", "prepare_attention"),
    "attn_bwd": ("attention_backward", "prepare_attention_backward"),
    "heads": ("attention_heads", "attention_backward_heads"),
}
LAUNCHES = {"sddmm", "sddmm_batch", "panels", "panels_local", "panels_one", "spmm", "spmm_t", "sddmm_backward",
            "softmax", "softmax_backward", "attention", "attention_backward", "attention_heads",
            "attention_backward_heads"}

Step = collections.namedtuple("Step", "family op args")


def st(family, op, **kw):
    return Step(family, op, tuple(sorted(kw.items())))


def arg(step, key, default=None):
    return dict(step.args).get(key, default)


def with_args(step, op=None, **kw):
    return Step(step.family, op or step.op, tuple(sorted(dict(step.args, **kw).items())))


# ------------------------------------------------------------------ the families' steps ----
def sddmm_ops():
    return [st("sddmm", "check"), st("sddmm", "stats"), st("sddmm", "prepare"),
            st("sddmm", "sddmm", data="exact"), st("sddmm", "sddmm", data="signed"),
            st("sddmm", "sddmm_batch", data="exact"), st("sddmm", "sddmm_batch", data="signed")]


def panels_ops():
    return [st("panels", "prepare_panels", r=0, local=False), st("panels", "panels", data="exact"),
            st("panels", "panels", data="signed"), st("panels", "prepare_panels", r=1, local=True),
            st("panels", "panels_local", data="exact"), st("panels", "panels_local", data="signed")]


def spmm_ops():
    return [st("spmm", "prepare_spmm", kd=0, sides=3, chunk=0), st("spmm", "spmm", kd=0, data="exact"),
            st("spmm", "spmm_t", kd=0, data="signed"), st("spmm", "sddmm_backward", kd=0, data="exact"),
            st("spmm", "prepare_spmm", kd=1, sides=3, chunk=32), st("spmm", "spmm", kd=1, data="signed"),
            st("spmm", "spmm_t", kd=1, data="exact"), st("spmm", "sddmm_backward", kd=1, data="signed"),
            st("spmm", "prepare_spmm", kd=1, sides=1, chunk=0), st("spmm", "spmm", kd=1, data="exact")]


def softmax_ops():
    return [st("softmax", "prepare_softmax"), st("softmax", "softmax", data="exact"),
            st("softmax", "softmax", data="signed"), st("softmax", "softmax_backward", data="exact"),
            st("softmax", "softmax_backward", data="signed")]


def attn_ops():
    return [st("attn", "prepare_attention", cfg=0), st("attn", "attention", cfg=0, data="exact", lse=True),
            st("attn", "attention", cfg=0, data="signed", lse=False),
            st("attn", "attention", cfg=1, data="exact", lse=False),
            st("attn", "attention", cfg=1, data="signed", lse=True), st("attn", "prepare_attention", cfg=1)]


def attn_bwd_ops():
    out = [st("attn_bwd", "prepare_attention_backward", cfg=0)]
    for i, want in enumerate(SUBSETS):  # every non-empty subset, both shapes, both data sets
        out.append(st("attn_bwd", "attention_backward", cfg=0 if i in (0, 4, 5, 6) else 1,
                      data="exact" if i % 2 == 0 else "signed", want=want))
    out += [st("attn_bwd", "attention_backward", cfg=1, data="exact", want=SUBSETS[0]),
            st("attn_bwd", "attention_backward", cfg=0, data="signed", want=SUBSETS[0])]
    return out


def heads_ops(backward_first=False):
    pairs = [(0, "exact", 0, SUBSETS[0]), (0, "signed", 1, SUBSETS[0]), (1, "exact", 1, ("GK", "GV")),
             (1, "signed", 2, SUBSETS[0]), (1, "exact", 2, ("GQ",))]
    out = []
    for cfg, data, bh, want in pairs:
        two = [st("heads", "attention_heads", cfg=cfg, data=data, bh=bh),
               st("heads", "attention_backward_heads", cfg=cfg, data=data, bh=bh, want=want)]
        out += two[::-1] if backward_first else two
    return out


FAMILY_OPS = {"sddmm": sddmm_ops, "panels": panels_ops, "spmm": spmm_ops, "softmax": softmax_ops, "attn": attn_ops,
              "attn_bwd": attn_bwd_ops, "heads": heads_ops}


def use(family, data, cfg=0):
    """One launch of the family."""
    return {"sddmm": st("sddmm", "sddmm", data=data), "panels": st("panels", "panels", data=data),
            "spmm": st("spmm", "sddmm_backward", kd=cfg, data=data), "softmax": st("softmax", "softmax", data=data),
            "attn": st("attn", "attention", cfg=cfg, data=data, lse=True),
            "attn_bwd": st("attn_bwd", "attention_backward", cfg=cfg, data=data, want=SUBSETS[0]),
            "heads": st("heads", "attention_heads", cfg=cfg, data=data, bh=0)}[family]


def refused(family, what):
    assert what in REFUSED[family]
    return st(family, "refused", what=what)


def recolumn(delta):
    assert delta in DELTAS
    return st("plan", "recolumn", delta=delta)


# the end of every sequence: back at the plan's own delta with one exact SDDMM, after which the
# plan must show the launch-path evidence of its sddmm_cases case (gpu_util.path_evidence)
CODA = [recolumn(0.3), st("sddmm", "sddmm", data="exact")]


def _first_use(order, backward_first):
    out = []
    for f in order:
        out += heads_ops(backward_first) if f == "heads" else FAMILY_OPS[f]()
    return out


def _recolumn_between():
    out = []
    for i, delta in enumerate((1.1, 0.0, 0.3)):
        out += [use(f, ("exact", "signed")[(i + j) % 2], cfg=i % 2) for j, f in enumerate(FAMILIES)]
        # the identity row list outlives the recolumn, the range layouts under it do not
        out += [recolumn(delta), st("panels", "panels_local", data=("exact", "signed")[i % 2])]
    return out + [use(f, "exact", cfg=1) for f in FAMILIES]


def _spmm_chunk_change():
    out = []
    for i, chunk in enumerate(CHUNKS):
        kd = 0 if i == 0 else 1
        out += [st("spmm", "prepare_spmm", kd=kd if i != 2 else 0, sides=3, chunk=chunk),
                st("spmm", "sddmm_backward", kd=kd, data="exact"), use("softmax", "signed"),
                st("spmm", "sddmm_backward", kd=0, data="signed"), use("attn", "exact", cfg=i % 2),
                st("spmm", "sddmm_backward", kd=1, data="exact")]
    return out


def _heads_between_singles():
    out = []
    for cfg, bh, data in ((0, 1, "exact"), (1, 0, "signed"), (1, 1, "exact"), (0, 1, "signed")):
        single = [st("attn", "attention", cfg=cfg, data=data, lse=True),
                  st("attn_bwd", "attention_backward", cfg=cfg, data=data, want=SUBSETS[0])]
        out += single + [st("heads", "attention_heads", cfg=cfg, data=data, bh=bh),
                         st("heads", "attention_backward_heads", cfg=cfg, data=data, bh=bh, want=SUBSETS[0])] + single
    return out


def _observers_first():
    out = [st("sddmm", "check"), st("sddmm", "stats"), st("sddmm", "sddmm", data="exact")]
    for delta in (0.0, 1.1, 0.3):
        out += [recolumn(delta), st("sddmm", "stats"), use("spmm", "exact"), st("sddmm", "check"),
                use("attn_bwd", "signed"), st("sddmm", "sddmm_batch", data="signed"), st("sddmm", "stats"),
                st("sddmm", "sddmm", data="exact")]
    return out


def _panel_cache_turnover():
    out = [st("panels", "prepare_panels", r=0, local=False), st("panels", "panels", data="exact")]
    others = [use("softmax", "exact"), use("spmm", "signed", cfg=1), use("attn", "exact"), use("heads", "signed"),
              use("attn_bwd", "exact", cfg=1), use("sddmm", "signed")]
    for i in range(N_CACHE_RANGES):
        out.append(st("panels", "panels_one", i=i, data="exact"))
        if i % 3 == 2:
            out.append(others[(i // 3) % len(others)])
    return out + [st("panels", "panels", data="signed"), st("panels", "panels_local", data="exact"),
                  st("panels", "panels_one", i=0, data="exact")]


def _refused_before_each():
    out = []
    for f in FAMILIES:
        out.append(use(f, "exact"))
        for what in REFUSED[f]:
            out += [refused(f, what), use(f, "signed" if what == "scale0" else "exact", cfg=1)]
    return out


def hand_written():
    """{name: [Step]}: one sequence per hazard, each ending in CODA."""
    seqs = {
        "first_use_forward": _first_use(FAMILIES, False),       # the backward borrows the forward's row lists
        "first_use_reverse": _first_use(FAMILIES[::-1], True),  # the backward is built first and owns them
        "recolumn_between": _recolumn_between(),
        "spmm_chunk_change": _spmm_chunk_change(),
        "heads_between_singles": _heads_between_singles(),
        "observers_first": _observers_first(),
        "panel_cache_turnover": _panel_cache_turnover(),
        "refused_before_each": _refused_before_each(),
    }
    return {k: v + CODA for k, v in seqs.items()}


def pool():
    """Every abstract step the random sequences draw from."""
    out = []
    for f in FAMILIES:
        out += FAMILY_OPS[f]()
        out += [refused(f, what) for what in REFUSED[f]]
    out += heads_ops(True)[:2]
    out += [st("panels", "panels_one", i=i, data="exact") for i in range(N_CACHE_RANGES)]
    out += [st("spmm", "prepare_spmm", kd=k, sides=s, chunk=c) for k in (0, 1) for s in (1, 2) for c in set(CHUNKS)]
    out += [recolumn(d) for d in DELTAS] * 2
    return out


RANDOM_SEEDS = (1, 2, 3, 4)
RANDOM_LENGTH = 40


def random_sequence(seed, n=RANDOM_LENGTH):
    rng = np.random.default_rng(seed)
    p = pool()
    return [p[int(i)] for i in rng.integers(0, len(p), n)] + CODA


# ------------------------------------------------------------- per plan: concrete steps ----
# name, the pattern (M, N, rowptr, colidx), the plan's own (K, dtype), row panels, and
# launch[(delta, K, dtype)] = (kind, row-block slot or -1) as the library decides it (a
# sddmm_cases kind; gpu_util.plan_launch of a plan at that delta)
Facts = collections.namedtuple("Facts", "name pat K dtype P launch")


def launch_keys(K, dtype):
    """The (delta, K, dtype) a Facts.launch must hold for a plan whose own SDDMM is (K, dtype)."""
    kds = {(K, dtype), (K, F32)} | set(PANEL_KD)
    return [(d, k, t) for d in DELTAS for (k, t) in sorted(kds)]


def sddmm_kd(facts, delta):
    """The (K, dtype) of the SDDMM family at `delta`: the plan's own, but fp32 while the column
    split would turn a plan of another kind into a dense-sampled one (that layout survives
    recolumn, and the plan's path evidence at the end names one launch kind)."""
    K, dt = facts.K, facts.dtype
    if dt != F32 and facts.launch[(0.3, K, dt)][0] != "dense" and facts.launch[(delta, K, dt)][0] == "dense":
        return K, F32
    return K, dt


def panel_kd(facts, delta, local):
    """((K, dtype), supported): the panel launches' operands at `delta`. Half operands and the
    local form need a row-block slot; without one the fp32 panel-major lists run (not local)."""
    slot = lambda kd: facts.launch[(delta,) + kd][1]  # noqa: E731
    own = sddmm_kd(facts, delta)
    if not local:
        return (own if slot(own) >= 0 or own[1] == F32 else (facts.K, F32)), True
    for kd in (own, (facts.K, F32)) + tuple(PANEL_KD):
        if slot(kd) >= 0:
            return kd, True
    return (facts.K, F32), False


def cache_ranges(P):
    """N_CACHE_RANGES distinct (index into PANEL_KD, p0, p1), none the whole plan: a layout each."""
    out = [(k, i, i + w) for w in range(1, P) for i in range(P - w + 1) for k in range(len(PANEL_KD))]
    assert len(out) >= N_CACHE_RANGES, f"{P} panels give only {len(out)} ranges"
    return out[:N_CACHE_RANGES]


def concrete(step, facts, delta):
    """The step with its (K, dtype) and panel ranges for this plan at the current delta."""
    f, op = step.family, step.op
    if op == "refused" or f in ("softmax", "plan"):
        return step
    if f == "sddmm":
        K, dt = sddmm_kd(facts, delta)
        return with_args(step, K=K, dtype=dt)
    if f == "panels":
        ranges = tuple(uneven_ranges(facts.P))
        if op == "panels_one":
            k, p0, p1 = cache_ranges(facts.P)[arg(step, "i")]
            return with_args(step, K=PANEL_KD[k][0], dtype=PANEL_KD[k][1], ranges=((p0, p1),))
        local = op == "panels_local" or bool(arg(step, "local"))
        (K, dt), ok = panel_kd(facts, delta, local)
        if op == "prepare_panels":
            return with_args(step, K=K, dtype=dt, ranges=(ranges[arg(step, "r")],), local=local and ok,
                             substituted=local and not ok)
        return with_args(step, op="panels_local" if local and ok else "panels", K=K, dtype=dt, ranges=ranges,
                         substituted=local and not ok)
    if f == "spmm":
        K, dt = SPMM_KD[arg(step, "kd")]
        return with_args(step, K=K, dtype=dt)
    D, Dv, dt = SHAPES[arg(step, "cfg")]
    B, H = HEADS_BH[arg(step, "bh")] if f == "heads" else (1, 1)
    return with_args(step, D=D, Dv=Dv, dtype=dt, slices=B * H)


# ---------------------------------------------------------------------------- the model ----
def _zeros(keys, **filled):
    return dict({k: 0 for k in keys}, **filled)


class Model:
    """The host-visible state of a plan after a sequence of concrete steps (module docstring)."""

    def __init__(self, facts, delta=0.3):
        self.f, self.delta = facts, delta
        self.rb = set()                  # whole-plan row-block layouts: (row bytes, half)
        self.ptile = self.dense = self.iota = False
        self.prep, self.lazy = [], []    # panel ranges, oldest first: (row bytes, half, p0, p1)
        self.spmm = {1: dict(built=False, chunk=0, K=0), 2: dict(built=False, chunk=0, K=0)}
        self.softmax = False
        self.attn = dict(built=False, floats=0)
        self.bwd = dict(built=False, shared=False, delta=0, row=0, col=0)
        self.largest = dict(spmm_K=0, attn_Dv=0, attn_slices=0, bwd_slices=0)
        self.attn_chunk = bsmr.attention_limits()["chunk"]
        self.bwd_lim = bsmr.attention_backward_limits()
        self._partials = {}

    def partials(self, side, chunk):
        key = (side, chunk)
        if key not in self._partials:
            self._partials[key] = PC.expected_stats(self.f.pat, side, chunk)["partials"]
        return self._partials[key]

    # ---- transitions
    def _launch(self, K, dtype):
        return self.f.launch[(self.delta, K, dtype)]

    def _whole(self, K, dtype):
        kind, _ = self._launch(K, dtype)
        if kind == "ptile":
            self.ptile = True
        elif kind == "dense":
            self.dense = True
        elif kind == "rowblock":
            self.rb.add((K * (4 if dtype == F32 else 2), dtype != F32))

    def _range(self, K, dtype, p0, p1, keep):
        _, slot = self._launch(K, dtype)
        if slot < 0 or p0 == p1:
            return
        key = (128 << slot, dtype != F32, p0, p1)
        if (p0, p1) == (0, self.f.P):
            self.rb.add(key[:2])
        elif key in self.prep or (key in self.lazy and not keep):
            return
        else:
            if key in self.lazy:
                self.lazy.remove(key)
            into = self.prep if keep else self.lazy
            if len(into) >= MAX_RANGES:
                del into[0]
            into.append(key)

    def _side(self, side, K, chunk):
        s = self.spmm[side]
        if not s["built"] or (chunk != 0 and chunk != s["chunk"]):
            s.update(built=True, chunk=chunk or PC.DEFAULT_CHUNK, K=0)
        if self.partials(side, s["chunk"]) and s["K"] < K:
            s["K"] = K
        self.largest["spmm_K"] = max(self.largest["spmm_K"], K)

    def _attention(self, Dv, slices):
        a = self.attn
        a["built"] = True
        a["floats"] = max(a["floats"], slices * self.partials(1, self.attn_chunk) * (Dv + 2))
        self.largest.update(attn_Dv=max(self.largest["attn_Dv"], Dv),
                            attn_slices=max(self.largest["attn_slices"], slices))

    def _backward(self, D, Dv, slices):
        b = self.bwd
        if not b["built"]:  # the forward's row lists are borrowed when they exist, else its own
            b.update(built=True, shared=self.attn["built"] and self.attn_chunk == self.bwd_lim["row_chunk"])
        b["delta"] = max(b["delta"], slices * self.f.pat[0])
        b["row"] = max(b["row"], slices * self.partials(1, self.bwd_lim["row_chunk"]) * D)
        b["col"] = max(b["col"], slices * self.partials(2, self.bwd_lim["col_chunk"]) * (D + Dv))
        self.largest["bwd_slices"] = max(self.largest["bwd_slices"], slices)

    def apply(self, c):
        """c: a concrete step. A refused call and stats() change nothing."""
        a, op = dict(c.args), c.op
        if op in ("refused", "stats"):
            return
        if op == "recolumn":  # drops what depends on the column split, keeps the rest
            self.delta = a["delta"]
            self.rb.clear()
            self.prep, self.lazy, self.ptile = [], [], False
        elif op in ("sddmm", "sddmm_batch", "prepare", "check"):
            self._whole(a["K"], a["dtype"])
        elif op in ("panels", "panels_local", "panels_one", "prepare_panels"):
            if op == "panels_local" or (op == "prepare_panels" and a["local"]):
                self.iota = True
            for p0, p1 in a["ranges"]:
                self._range(a["K"], a["dtype"], p0, p1, keep=op == "prepare_panels")
        elif op == "spmm":
            self._side(1, a["K"], 0)
        elif op == "spmm_t":
            self._side(2, a["K"], 0)
        elif op == "sddmm_backward":
            self._side(1, a["K"], 0)
            self._side(2, a["K"], 0)
        elif op == "prepare_spmm":
            for side in (1, 2):
                if a["sides"] & side:
                    self._side(side, a["K"], a["chunk"])
        elif op in ("softmax", "softmax_backward", "prepare_softmax"):
            self.softmax = True
        elif op in ("attention", "prepare_attention", "attention_heads"):
            self._attention(a["Dv"], a["slices"])
        elif op in ("attention_backward", "prepare_attention_backward", "attention_backward_heads"):
            self._backward(a["D"], a["Dv"], a["slices"])
        else:
            raise KeyError(op)

    # ---- what the queries must answer
    def sddmm_prepared(self, K, dtype):
        kind, _ = self._launch(K, dtype)
        if kind in ("half", "colmajor"):
            return True
        if kind == "ptile":
            return self.ptile
        if kind == "dense":
            return self.dense
        return (K * (4 if dtype == F32 else 2), dtype != F32) in self.rb

    def panels_prepared(self, K, dtype, p0, p1, local):
        _, slot = self._launch(K, dtype)
        if slot < 0:
            return not local and dtype == F32  # (else the call itself is unsupported)
        if local and not self.iota:
            return False
        key = (128 << slot, dtype != F32, p0, p1)
        if (p0, p1) == (0, self.f.P):
            return key[:2] in self.rb
        return key in self.prep or key in self.lazy

    def spmm_prepared(self, K, sides):
        return all(self.spmm[s]["built"] and (self.partials(s, self.spmm[s]["chunk"]) == 0 or self.spmm[s]["K"] >= K)
                   for s in (1, 2) if sides & s)

    def attention_prepared(self, D, Dv, slices=1):
        return self.attn["built"] and self.attn["floats"] >= slices * self.partials(1, self.attn_chunk) * (Dv + 2)

    def backward_prepared(self, D, Dv, slices=1):
        b, lim = self.bwd, self.bwd_lim
        return (b["built"] and b["delta"] >= slices * self.f.pat[0] and
                b["row"] >= slices * self.partials(1, lim["row_chunk"]) * D and
                b["col"] >= slices * self.partials(2, lim["col_chunk"]) * (D + Dv))

    def query_keys(self):
        f = self.f
        kds = sorted({(f.K, f.dtype), (f.K, F32)})
        keys = [("sddmm", K, dt) for K, dt in kds]
        for K, dt in sorted(set(kds) | set(PANEL_KD)):
            keys += [("panels", K, dt, p0, p1, local) for p0, p1 in uneven_ranges(f.P) for local in (False, True)]
        keys += [("panels", PANEL_KD[k][0], PANEL_KD[k][1], p0, p1, False) for k, p0, p1 in cache_ranges(f.P)]
        keys += [("spmm", K, sides) for K, _ in SPMM_KD for sides in (1, 2, 3)]
        keys.append(("softmax",))
        slices = sorted({b * h for b, h in HEADS_BH})
        keys += [(fam, D, Dv, z) for fam in ("attn", "bwd") for D, Dv, _ in SHAPES for z in slices]
        return keys

    def answer(self, key):
        fn = {"sddmm": self.sddmm_prepared, "panels": self.panels_prepared, "spmm": self.spmm_prepared,
              "softmax": lambda: self.softmax, "attn": self.attention_prepared, "bwd": self.backward_prepared}[key[0]]
        return bool(fn(*key[1:]))

    def prepared(self):
        return {k: self.answer(k) for k in self.query_keys()}

    def stats(self):
        """What spmm_stats(1), spmm_stats(2), softmax_stats, attention_stats and
        attention_backward_stats must return: zeros (and the always-filled constants) until built."""
        pat = self.f.pat
        out = {}
        for side in (1, 2):
            s = self.spmm[side]
            out[f"spmm{side}"] = (PC.expected_stats(pat, side, s["chunk"]) if s["built"] else
                                  _zeros(("segments", "split_dsts", "partials", "max_list", "chunk")))
        out["softmax"] = SC.expected_stats(pat) if self.softmax else _zeros(
            ("items", "packed_runs", "wave_rows", "block_rows", "max_row"), **SC.limits())
        e = PC.expected_stats(pat, 1, self.attn_chunk)
        out["attn"] = (dict(segments=e["segments"], split_rows=e["split_dsts"], partials=e["partials"],
                            max_row=e["max_list"], chunk=self.attn_chunk) if self.attn["built"] else
                       _zeros(("segments", "split_rows", "partials", "max_row"), chunk=self.attn_chunk))
        b = BC.expected_stats(pat, built=self.bwd["built"])
        b.update(row_scratch_bytes=4 * self.bwd["row"], col_scratch_bytes=4 * self.bwd["col"],
                 delta_bytes=4 * self.bwd["delta"])
        out["bwd"] = b
        return out


def run_model(facts, steps, delta=0.3):
    """(model after the steps, the concrete steps)."""
    m, out = Model(facts, delta), []
    for s in steps:
        c = concrete(s, facts, m.delta)
        m.apply(c)
        out.append(c)
    return m, out


def projection(steps, family):
    """The steps a fresh plan of `family` receives: the family's own and every recolumn."""
    return [s for s in steps if s.family == family or s.op == "recolumn"]


# ------------------------------------------------------------------- the bit comparison ----
def bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32, x.dtype
    return x.view(np.uint32)


def same_bits(a, b):
    """Bit for bit: the sign of a zero and the payload of a NaN count."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def assert_same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} and {b.shape}"
    bad = np.nonzero((bits(a) != bits(b)).ravel())[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {a.size} elements differ bit for bit, first at {bad[:5]}: "
                           f"{a.ravel()[bad[:5]]} against {b.ravel()[bad[:5]]}")
