"""The store pass of the row-block SDDMM (how an item's results get from LDS to P), restated in
numpy: the run cutting, the store forms, the classification of a launch by the form each
workgroup takes, and the table STORE_CASES of tests/test_gpu_sddmm_store_float64.py (no GPU here:
tests/test_store_ref_cpu.py checks this module).

A staged row-block layout (csrc/plan.hpp RowBlockLayout::outLds != 0) keeps each item's results
in LDS slots, slot t = the item's t-th entry by CSR position, and writes them to P at the end of
the item. csrc/rb_kernel.hpp has these forms of that pass (the store passes of
k_sddmm_rb and of the pair's rb_item, store_sorted):

  R  run table (outRuns): the slots cut into runs of up to 64 consecutive positions, descriptor
     {position, slot | length << 16}; lane l of wave w holds run w + NW l; a wave stores its runs
     four per step, lane < length storing P[position + lane] = slot[first + lane]
  S  sortedPos (no run table: some item has more runs than the workgroup has threads, NT): thread
     t stores slots t, t + NT, ..., eight per trip of 8 NT slots, P[sortedPos[first + s]] = slot[s]
  P  pairs (k_sddmm_rb_pair; run table only): a workgroup runs list positions 2 j and 2 j + 1 of
     its XCD. The first item of a pair with a real partner and at most NW PAIR_RUNS_PER_WAVE runs
     takes the register path (run values to registers, barrier, the partner's image staged over the
     slot tail unless it is the same row block, then the stores); with more runs, the plain path
     (form R, then a barrier and the staging); a first item whose partner is padding, and every
     second item, store as form R.

Evidence (classify): what a launch of a dumped layout runs, from the tables alone. `dump` is the
dict of gpu_util.rb_store (the library's exports bsmr_debug_rb_store and bsmr_debug_rb_pieces) or
of a host-only model of the layout (tests/test_store_ref_cpu.py): header words, per item slot its
entries / runs / longest / shortest run, its row block and whether it is padding, the raw tables.
The constants (PAIR_RUNS_PER_WAVE, XCD_BUCKETS) come from the library with the dump.

  R-idle   an item with fewer runs than waves: some waves have no run
  R-steps  an item with more than 4 NW runs and a wave whose run count is no multiple of 4: more
           than one four-run step, the last one partial
  R-64     a run of length 64 directly followed by a run that starts at the next position
  R-1      runs of length 1 and of a length in (1, 64) in one item
  R-tail   an item whose entries exceed half of outCap (the slots reach deep into the LDS tail)
  S-trips  an item with more than 8 NT entries, the count no multiple of NT: a second trip, ragged
  S-small  an item with fewer than NT entries
  P-reg-same / P-reg-stage   register path, the partner in the same / another row block
  P-reg-stage-tail           P-reg-stage by a first item that is also R-tail: the partner's image
                             (its filler blocks) lands on slots that were just read
  P-plain-same / P-plain-stage   plain path inside a pair with a real partner
  P-last   the partner is padding
"""
import collections
import ctypes as C

import numpy as np

import bsmr
from bsmr import BF16, F16, F32

RUN_MAX = 64   # lanes of a wave: the longest run (csrc/rb_schedule.hpp RB_RUN_MAX)
STEP = 4       # runs a wave stores per step
TRIP = 8       # slots a thread stores per trip of the sortedPos form

_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")


# ---- the run cutting ------------------------------------------------------------------------------

def cut_runs_ref(sorted_pos, ient, NT, cut=RUN_MAX):
    """The run table as csrc/rb_schedule.hpp documents it, restated: every item's maximal sequences
    of consecutive positions, each chopped into pieces of `cut`. ient: (n, 2) {first entry,
    entries}. Returns dict(fits, itemRuns (n, 2), runs (r, 2) or empty when not fits)."""
    sorted_pos = np.asarray(sorted_pos, np.int64)
    item_runs, runs = [], []
    for e0, ln in np.asarray(ient, np.int64).reshape(-1, 2):
        pos = sorted_pos[e0:e0 + ln]
        first = len(runs)
        if ln:
            brk = np.nonzero(np.diff(pos) != 1)[0] + 1
            for a, b in zip(np.concatenate([[0], brk]), np.concatenate([brk, [ln]])):
                for t in range(a, b, cut):
                    runs.append((pos[t], t | (min(cut, b - t) << 16)))
        item_runs.append((first, len(runs) - first))
    item_runs = np.array(item_runs, np.uint32).reshape(-1, 2)
    fits = bool((item_runs[:, 1] <= NT).all())
    return dict(fits=fits, itemRuns=item_runs,
                runs=np.array(runs if fits else [], np.uint32).reshape(-1, 2))


def cut_runs(sorted_pos, ient, NT, threads=0):
    """The same through the library's host-only export bsmr_debug_rb_runs (no device)."""
    f = bsmr.lib().bsmr_debug_rb_runs
    f.argtypes = [_u32p, C.c_uint64, _u32p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p,
                  C.POINTER(C.c_uint64)]
    sorted_pos = np.ascontiguousarray(sorted_pos, np.uint32).reshape(-1)
    ient = np.ascontiguousarray(ient, np.uint32).reshape(-1, 2)
    args = (sorted_pos if len(sorted_pos) else np.zeros(1, np.uint32), len(sorted_pos),
            ient.reshape(-1) if len(ient) else np.zeros(2, np.uint32), len(ient), NT, threads)
    n = C.c_uint64()
    assert f(*args, None, C.byref(n)) == 0, bsmr.lib().bsmr_last_error()
    buf = np.zeros(n.value, np.uint32)
    assert f(*args, buf.ctypes.data, C.byref(n)) == 0
    ni, nr = int(buf[1]), int(buf[2])
    assert ni == len(ient) and len(buf) == 3 + 2 * ni + 2 * nr
    return dict(fits=bool(buf[0]), itemRuns=buf[3:3 + 2 * ni].reshape(-1, 2),
                runs=buf[3 + 2 * ni:].reshape(-1, 2))


# ---- the store passes -----------------------------------------------------------------------------

# what a subtly wrong kernel (or table) would do; each must fail assert_exact on identity data
MUTATIONS = ("run_length_minus_one", "lane_equal_to_len_stores", "last_partial_step_dropped",
             "second_trip_dropped", "cut_at_65", "slot_of_neighbouring_run")


def store_by_runs(P, res, runs, NT, mutation=None):
    """Form R on one item: res = its slots, runs = its (r, 2) descriptors. Lane l of wave w holds
    run w + NW l; wave w has nr = ceil((r - w) / NW) of them and stores them STEP per step."""
    NW = NT // 64
    r = len(runs)
    lane = np.arange(64)
    for w in range(NW):
        nr = (r - w + NW - 1) // NW if r > w else 0
        mine = np.zeros((64, 2), np.int64)  # the wave's descriptor registers, {0, 0} past the item's
        idx = w + NW * lane
        mine[idx < r] = runs[idx[idx < r]]
        steps = range(0, nr - nr % STEP if mutation == "last_partial_step_dropped" else nr, STEP)
        for i in steps:
            for u in range(STEP):
                q = min(i + u, 63)
                pos, sl = mine[q]
                s0, ln = sl & 0xFFFF, (sl >> 16 if i + u < nr else 0)
                if mutation == "slot_of_neighbouring_run" and ln and nr > 1:
                    s0 = mine[q + 1 if i + u + 1 < nr else q - 1][1] & 0xFFFF
                if mutation == "run_length_minus_one":
                    ln = max(ln - 1, 0)
                on = lane <= ln if mutation == "lane_equal_to_len_stores" and ln else lane < ln
                src = s0 + lane[on]
                ok = src < len(res)  # (a read past the item's slots: whatever the LDS holds)
                dst = pos + lane[on]
                P[dst[ok]] = res[src[ok]]
                P[dst[~ok]] = -1.0


def store_by_positions(P, res, pos, NT, mutation=None):
    """Form S on one item: thread t stores slots t + k NT of every trip of TRIP NT slots."""
    n = len(res)
    tid = np.arange(NT)
    trips = range(0, n, TRIP * NT)
    for t0 in (list(trips)[:1] if mutation == "second_trip_dropped" else trips):
        for k in range(TRIP):
            t = t0 + tid + k * NT
            t = t[t < n]
            P[pos[t]] = res[t]


def emulate(dump, sorted_pos, values, mutation=None, reverse=False, guard=1):
    """P (float64, NaN where nothing was stored, `guard` extra elements past the end) of the store
    passes of every real item of `dump`, in launch order (reverse: backwards; workgroups are not
    ordered among themselves). sorted_pos: every item's positions in slot order (the input of the
    run cutting); values: the result per CSR position. A run-table layout stores by its runs
    (mutation "cut_at_65": by the table cut at 65, still with 64 lanes), else by sortedPos."""
    values = np.asarray(values, np.float64)
    P = np.full(len(values) + guard, np.nan)
    if not dump["outLds"]:
        raise ValueError("the layout is not staged: nothing to emulate")
    ient = np.asarray(dump["itemEnt"], np.int64)
    NT = dump["NT"]
    runs_tab = None
    if dump["outRuns"]:
        runs_tab = (cut_runs_ref(sorted_pos, ient, NT, cut=65) if mutation == "cut_at_65"
                    else dict(itemRuns=dump["itemRuns"], runs=dump["runs"]))
    order = range(len(ient))
    for i in (reversed(order) if reverse else order):
        e0, n = ient[i]
        if not dump["real"][i] or n == 0:
            continue
        pos = np.asarray(sorted_pos[e0:e0 + n], np.int64)
        res = values[pos]
        if runs_tab is not None:
            r0, nr = (int(x) for x in runs_tab["itemRuns"][i])
            store_by_runs(P, res, np.asarray(runs_tab["runs"][r0:r0 + nr], np.int64), NT, mutation)
        else:
            store_by_positions(P, res, pos, NT, mutation)
    return P


# ---- what a launch runs ---------------------------------------------------------------------------

def wave_run_counts(nruns, NW):
    """Runs of each wave of an item of nruns runs (run j goes to wave j % NW)."""
    w = np.arange(NW)
    return np.where(nruns > w, (nruns - w + NW - 1) // NW, 0)


def classify(dump, pairs):
    """(evidence: set of the names of the module docstring plus the form "direct" / "R" / "S" / "P"
    and "NT512" / "NT1024"; facts: dict(max_entries, outCap, fill = max_entries / outCap, items,
    max_runs)) of a launch of `dump` as single items (pairs false) or as pairs."""
    ev = {f"NT{dump['NT']}"}
    real = np.asarray(dump["real"], bool)
    ent = np.asarray(dump["ent"], np.int64)
    facts = dict(items=int(real.sum()), max_entries=int(ent[real].max(initial=0)), outCap=int(dump["outCap"]),
                 max_runs=int(np.asarray(dump["nruns"])[real].max(initial=0)))
    facts["fill"] = facts["max_entries"] / facts["outCap"] if facts["outCap"] else 0.0
    if not dump["outLds"]:
        assert not pairs
        ev.add("direct")
        return ev, facts
    NT, cap = dump["NT"], dump["outCap"]
    NW = NT // 64
    if not dump["outRuns"]:
        assert not pairs, "pairs without a run table"
        ev.add("S")
        e = ent[real]
        if ((e > TRIP * NT) & (e % NT != 0)).any():
            ev.add("S-trips")
        if ((e > 0) & (e < NT)).any():
            ev.add("S-small")
        return ev, facts
    nruns = np.asarray(dump["nruns"], np.int64)
    tail = 2 * ent > cap
    if pairs:
        ev.add("P")
        X = dump["xcds"]
        lim = NW * dump["prpw"]
        n = len(real)
        assert n % (2 * X) == 0
        for g in range(n // 2):
            a = (g // X) * 2 * X + g % X
            b = a + X
            if not real[a]:
                assert not real[b], "padding before a real item in an XCD's list"
                continue
            if not real[b]:
                ev.add("P-last")
                continue
            same = dump["rb"][a] == dump["rb"][b]
            if nruns[a] <= lim:
                ev.add("P-reg-same" if same else "P-reg-stage")
                if not same and tail[a]:
                    ev.add("P-reg-stage-tail")
            else:
                ev.add("P-plain-same" if same else "P-plain-stage")
        return ev, facts
    ev.add("R")
    if dump.get("runs") is None:
        raise ValueError("the run words are needed to classify a run-table launch")
    irun = np.asarray(dump["itemRuns"], np.int64)
    runs = np.asarray(dump["runs"], np.int64)
    for i in np.nonzero(real & (ent > 0))[0]:
        r = nruns[i]
        if r < NW:
            ev.add("R-idle")
        if r > STEP * NW and (wave_run_counts(r, NW) % STEP != 0).any():
            ev.add("R-steps")
        if tail[i]:
            ev.add("R-tail")
        mine = runs[irun[i, 0]:irun[i, 0] + r]
        ln = mine[:, 1] >> 16
        if (ln == 1).any() and ((ln > 1) & (ln < RUN_MAX)).any():
            ev.add("R-1")
        if ((ln[:-1] == RUN_MAX) & (mine[1:, 0] == mine[:-1, 0] + RUN_MAX)).any():
            ev.add("R-64")
    return ev, facts


def host_rule(dump):
    """build_output_tables' choice restated on a staged dump that still holds its positions (form
    S): the run table is used iff no item has more runs than NT, outCap < 65536 (and no diag bit).
    Returns (run table wanted, the most runs of an item)."""
    t = cut_runs_ref(dump["sortedPos"], dump["itemEnt"], dump["NT"])
    most = int(t["itemRuns"][:, 1].max(initial=0))
    return t["fits"] and dump["outCap"] < 65536, most


# ---- the cases of tests/test_gpu_sddmm_store_float64.py -------------------------------------------

# name, pattern (sddmm_cases.pattern), K, dtype, tuning, whether the launch pairs, the evidence the
# launch must show (classify), and whether the host-only model of test_store_ref_cpu.py applies
# (original-order row blocks: the layout follows from the CSR alone, so the evidence is checked
# without a GPU too)
StoreCase = collections.namedtuple("StoreCase", "name pattern K dtype tuning pairs evidence model")

STAGED = {"out_staged": 1, "tile_min_half": 257}
# `band` (215,552 entries) and piece_weight = 4096: an item's modelled cost is then its number of
# column-run pieces, so the scattered rows (one piece per entry) set the cost of an item and the
# items of the dense band (16 entries per piece) hold 16 times the entries: the large items that
# R-tail, S-trips and P-reg-stage-tail need. DESIGN.md §5 derives why no smaller pattern has them
BAND = dict(STAGED, orig_rows=1, piece_weight=4096.0)


def _store_cases():
    out = []

    def add(name, pattern, K, dtype, tuning, evidence, pairs=False, model=False):
        ev = set(evidence.split())
        assert not model or tuning.get("orig_rows") == 1
        out.append(StoreCase(name, pattern, K, dtype, dict(tuning), pairs, ev, model))

    # --- the run table, single items
    # few entries per item (the reordered layout of the small patterns): idle waves, short runs
    add("runs_zipf_rb16", "zipf", 128, F32, dict(STAGED, rb_rows=16), "R NT512 R-idle R-1")
    add("runs_hub_rb16", "hub", 128, F32, dict(STAGED, rb_rows=16), "R NT512 R-idle R-1")
    add("runs_uniform300_rb16", "uniform300", 128, F32, dict(STAGED, rb_rows=16), "R NT512 R-1")
    # the same pattern with unsorted rows still fits the table: one run per entry
    add("runs_zipf_shuffled_rb144", "zipf_shuffled", 128, F32, dict(STAGED, rb_rows=144), "R NT512 R-steps R-1")
    add("runs_zipf_rb288", "zipf", 128, F32, dict(STAGED, rb_rows=288), "R NT1024 R-steps R-1")
    add("runs_zipf_orig_rb16", "zipf", 128, F32, dict(STAGED, orig_rows=1, rb_rows=16), "R NT512 R-idle R-1",
        model=True)
    # large items
    add("runs_band_rb64", "band", 128, F32, dict(BAND, rb_rows=64), "R NT512 R-steps R-64 R-1", model=True)
    add("runs_band_rb144", "band", 128, F32, dict(BAND, rb_rows=144), "R NT512 R-steps R-1 R-tail", model=True)
    add("runs_band_rb288", "band", 128, F32, dict(BAND, rb_rows=288), "R NT1024 R-steps R-1 R-tail", model=True)
    add("runs_band_bf16_rb144", "band", 256, BF16, dict(BAND, rb_rows=144), "R NT512 R-steps R-1 R-tail",
        model=True)
    add("runs_band_2k_rb32", "band", 512, F32, dict(BAND, rb_rows=32), "R NT512 R-64 R-1 R-tail", model=True)
    # --- sortedPos: an unsorted pattern whose large items have more runs than threads
    add("pos_band_rb64", "band_shuffled", 128, F32, dict(BAND, rb_rows=64, pair_min_items=0),
        "S NT512 S-trips S-small", model=True)
    add("pos_band_rb288", "band_shuffled", 128, F32, dict(BAND, rb_rows=288, pair_min_items=0),
        "S NT1024 S-small", model=True)
    add("pos_band_f16_rb64", "band_shuffled", 256, F16, dict(BAND, rb_rows=64, pair_min_items=0),
        "S NT512 S-trips S-small", model=True)
    # the same pattern under the default cost model (no piece_weight): items of up to ~2000 entries,
    # still more runs than threads; no second trip
    add("pos_band_default_weight_rb64", "band_shuffled", 128, F32,
        dict(STAGED, orig_rows=1, rb_rows=64, pair_min_items=0), "S NT512 S-small", model=True)
    # --- pairs
    add("pair_zipf_rb16", "zipf", 128, F32, dict(STAGED, rb_rows=16, pair_min_items=0),
        "P NT512 P-reg-same P-reg-stage", pairs=True)
    add("pair_band_rb144", "band", 128, F32, dict(BAND, rb_rows=144, pair_min_items=0),
        "P NT512 P-reg-same P-reg-stage P-reg-stage-tail P-plain-same P-plain-stage P-last", pairs=True,
        model=True)
    add("pair_band_rb288", "band", 128, F32, dict(BAND, rb_rows=288, pair_min_items=0),
        "P NT1024 P-reg-same P-reg-stage P-reg-stage-tail P-plain-same P-plain-stage", pairs=True, model=True)
    add("pair_dyn_band_rb144", "band", 128, F32, dict(BAND, rb_rows=144, pair_min_items=0, batches=1),
        "P NT512 P-reg-stage P-reg-stage-tail P-plain-stage P-last", pairs=True, model=True)
    # --- column blocks, staged, on an unsorted pattern: an item's slots are runs down a column of
    # S, so its CSR positions are scattered whatever the order inside a row (one run per entry, and
    # few enough of them for the table)
    add("cols_zipf_shuffled", "zipf_shuffled", 128, F32, dict(STAGED, col_blocks=1), "R NT1024 R-steps R-1")
    assert len({c.name for c in out}) == len(out)
    return out


STORE_CASES = _store_cases()
STORE_BY_NAME = {c.name: c for c in STORE_CASES}
# the other entry points (bsmr_sddmm_batch with three batches, bsmr_sddmm_panels over three uneven
# ranges), once through each store form
STORE_ENTRY_CASES = ["runs_zipf_rb16", "pos_band_rb64", "pair_band_rb144"]
# bsmr_sddmm_panels runs a layout of each range's own (reordered rows; orig_rows does not apply):
# the evidence that must show among the three uneven ranges, read from the range layouts
# (pos_band_rb64: the range that holds the band's rows keeps sortedPos, the other two fit the run
# table and pair_min_items = 0 pairs them)
STORE_PANEL_CASES = {"runs_zipf_rb16": set("R NT512 R-idle R-1".split()),
                     "pos_band_rb64": set("S S-small P P-reg-same P-reg-stage".split()),
                     "pair_band_rb144": set("P P-reg-same P-reg-stage P-plain-same".split())}
# one sorted pattern with BSMR_DIAG & 8192 (the run table switched off): form S on a layout whose
# run-table twin exists, so the two results must agree bit for bit on signed data
DIAG_TWIN = ("runs_band_rb64", 8192)


def as_case(sc):
    """The sddmm_cases.Case of a StoreCase (for plan_kwargs, path_evidence, check_stats)."""
    from sddmm_cases import Case, DTYPE_NAME
    proof = {"rb_pairs": sc.pairs, "nt": 1024 if "NT1024" in sc.evidence else 512,
             "store": "positions" if "S" in sc.evidence else "runs",
             "rb_col_blocks": sc.tuning.get("col_blocks") == 1}
    if sc.tuning.get("orig_rows") == 1:
        proof["rb_orig_rows"] = True
    if "batches" in sc.tuning:
        proof["rb_batches"] = sc.tuning["batches"] == 1
    return Case(f"{sc.name}_K{sc.K}_{DTYPE_NAME[sc.dtype]}", "rowblock", sc.pattern, sc.K, sc.dtype, "auto",
                dict(sc.tuning), proof, None)
