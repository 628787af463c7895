"""CPU: the host-only row-block scheduler (csrc/rb_schedule.cpp) through its two device-free debug
exports, bsmr_debug_rb_geometry and bsmr_debug_rb_schedule.

For original-order and column-block layouts the scheduler's input follows from the CSR alone: an
entry's block is row // RB (col // RB for column blocks), entries are sorted by block, then by
column (row for column blocks), ties in CSR order (the device radix sort is stable). So the
layouts recorded on the GPU (tests/golden/mi355x_rb_layout_digests.json) can be reproduced here.
"""
import ctypes as C

import numpy as np
import pytest

import bsmr
import rb_layout_cases as R
from bsmr import synth

CM = (1 << 22) - 1
GEOM = ["rowBytes", "orig", "cols", "RB", "NT", "nRB", "lds", "l2Kb", "m", "stagedWanted", "staged",
        "outCap", "perBucket"]
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")


def _tuning_ptr(tuning):
    return C.byref(bsmr._tuning_struct(tuning or {}))


def geometry(row_bytes, Rs, n0, NS, nnz, cus, orig=False, cols=False, tuning=None):
    f = bsmr.lib().bsmr_debug_rb_geometry
    f.argtypes = [C.c_uint32] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_int, _u32p]
    out = np.zeros(len(GEOM), np.uint32)
    assert f(row_bytes, Rs, n0, NS, nnz, int(orig), int(cols), _tuning_ptr(tuning), cus, out) == 0
    return out


def schedule(cols_sorted, rb_end, geom, NS, kept=None, tuning=None, threads=0):
    """{items (n x 4), ends, pieces (p x 2), stat (n x 4), dyn, work} of bsmr_debug_rb_schedule."""
    f = bsmr.lib().bsmr_debug_rb_schedule
    f.argtypes = [C.c_void_p, C.c_uint64, _u32p, C.c_void_p, C.c_uint32, _u32p, C.c_void_p, C.c_int,
                  C.c_void_p, C.POINTER(C.c_uint64)]
    cols_sorted = np.ascontiguousarray(cols_sorted, np.uint32)
    rb_end = np.ascontiguousarray(rb_end, np.uint32)
    geom = np.ascontiguousarray(geom, np.uint32)
    kept = None if kept is None else np.ascontiguousarray(kept, np.uint32)
    args = (cols_sorted.ctypes.data, len(cols_sorted), rb_end, None if kept is None else kept.ctypes.data,
            NS, geom, _tuning_ptr(tuning), threads)
    n = C.c_uint64()
    assert f(*args, None, C.byref(n)) == 0
    buf = np.zeros(n.value, np.uint32)
    assert f(*args, buf.ctypes.data, C.byref(n)) == 0
    ni, p = int(buf[0]), int(buf[1])
    assert len(buf) == 4 + 9 * ni + 2 * p
    o = 2
    items = buf[o:o + 4 * ni].reshape(-1, 4)
    o += 4 * ni
    ends = buf[o:o + ni]
    o += ni
    pieces = buf[o:o + 2 * p].reshape(-1, 2)
    o += 2 * p
    stat = buf[o:o + 4 * ni].reshape(-1, 4)
    o += 4 * ni
    return {"items": items, "ends": ends, "pieces": pieces, "stat": stat, "dyn": int(buf[o]),
            "work": int(buf[o + 1]), "raw": buf}


def csr_input(M, N, rp, ci, RB, nRB, cols):
    """The sorted "columns" and rbEnd of an original-order (cols: column-block) layout."""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(rp))
    block, gathered = (ci // RB, rows) if cols else (rows // RB, ci)
    order = np.lexsort((gathered, block))  # stable: ties stay in CSR order
    rb_end = np.cumsum(np.bincount(block, minlength=nRB))[:nRB]
    return gathered[order].astype(np.uint32), rb_end.astype(np.uint32)


def csr_layout(pattern, K, tuning, cols, cus, threads=0):
    M, N, rp, ci = pattern
    Rs, NS = (N, M) if cols else (M, N)
    g = geometry(4 * K, Rs, len(ci), NS, len(ci), cus, orig=not cols, cols=cols, tuning=tuning)
    G = dict(zip(GEOM, (int(v) for v in g)))
    e, rb_end = csr_input(M, N, rp, ci, G["RB"], G["nRB"], cols)
    return G, e, schedule(e, rb_end, g, NS, tuning=tuning, threads=threads)


# ---- equivalence with the layouts recorded on the GPU -------------------------------------------

CSR_CASES = {"plan_check/orig_rows": False, "plan_check/batches_orig": False,
             "trefethen3000/orig_not_contig": False,
             "trefethen3000/orig_round2_rb16": False, "wide/col_blocks": True,
             "cols_local/col_blocks": True}


@pytest.mark.parametrize("name", sorted(CSR_CASES))
def test_reproduces_the_recorded_gpu_layout(name):
    gold = R.load_golden()
    pat, K, dtype, kw = R.CASES[name]
    assert dtype == bsmr.F32
    G, _, s = csr_layout(pat(), K, kw.get("tuning"), CSR_CASES[name], gold["cus"])
    words = R.layout_words(G["RB"], G["NT"], G["rowBytes"], s["items"], s["ends"], s["pieces"])
    assert R.digest(words) == gold["digests"][name]


# ---- invariants ---------------------------------------------------------------------------------

def check_invariants(e, s, piece_max=16, longest_first=True):
    n, items, ends, pieces = len(e), s["items"], s["ends"], s["pieces"]
    plen = (pieces[:, 1] >> 22).astype(np.int64) + 1
    # items partition the pieces, pieces partition the entries
    real = ends > items[:, 3]
    owner = np.zeros(len(pieces), np.int64)
    for i in np.nonzero(real)[0]:
        owner[items[i, 3]:ends[i]] += 1
    assert (owner == 1).all(), "a piece outside every item, or in two"
    cover = np.zeros(n + 1, np.int64)
    np.add.at(cover, pieces[:, 0], 1)
    np.add.at(cover, pieces[:, 0] + plen, -1)
    assert (np.cumsum(cover)[:n] == 1).all() and plen.sum() == n, "an entry in no piece, or in two"
    assert plen.max(initial=0) <= piece_max
    for (e0, w), ln in zip(pieces, plen):
        assert (e[e0:e0 + ln] == (w & CM)).all(), "a piece spans two columns"
    assert int(s["stat"][:, 2].sum()) == n
    assert int(s["stat"][:, 3].sum()) == len(pieces)
    assert s["work"] == int(((items[:, 1] != items[:, 2]) | real).sum())
    if longest_first:
        for i in np.nonzero(real)[0]:
            assert (np.diff(plen[items[i, 3]:ends[i]]) <= 0).all(), f"item {i} not longest first"


def hand_input():
    """3 row blocks of 16 rows: mixed columns; one column 40 times (pieces 16, 16, 8); empty."""
    b0 = np.sort(np.array([0, 0, 0, 3, 3, 7, 9, 9, 9, 9, 20, 31, 31, 63], np.uint32))
    b1 = np.full(40, 5, np.uint32)
    e = np.concatenate([b0, b1])
    rb_end = np.array([len(b0), len(e), len(e)], np.uint32)
    geom = np.array([256, 1, 0, 16, 512, 3, 16 * 256, 2048, 1, 0, 0, (80 * 1024 - 4096 - 16) // 4, 64],
                    np.uint32)
    return e, rb_end, geom, 64


def test_invariants_hand_made():
    e, rb_end, geom, NS = hand_input()
    # default tuning: the cost cap (a share of 512 slots) cuts these few entries into many items
    check_invariants(e, schedule(e, rb_end, geom, NS))
    # no cap: one item per non-empty block
    s = schedule(e, rb_end, geom, NS, tuning={"item_cap": 0})
    assert not s["dyn"] and s["work"] == 2
    check_invariants(e, s)
    b1 = s["pieces"][s["pieces"][:, 0] >= rb_end[0]]
    assert sorted((b1[:, 1] >> 22) + 1) == [8, 16, 16] and ((b1[:, 1] & CM) == 5).all()
    assert set(s["stat"][s["stat"][:, 2] > 0][:, 0]) == {0, 1}  # the empty block has no item
    s4 = schedule(e, rb_end, geom, NS, tuning={"item_cap": 0, "piece_max": 4})
    check_invariants(e, s4, piece_max=4)
    assert len(s4["pieces"]) == 7 + 10  # 7 columns of <= 4 entries in block 0, 40 / 4 in block 1


def test_invariants_trefethen_orig():
    G, e, s = csr_layout(synth.trefethen(3000), 64, {"batches": 0}, False, 256)
    assert not s["dyn"] and G["nRB"] > 8
    check_invariants(e, s)


def test_invariants_column_blocks():
    G, e, s = csr_layout(synth.random_rows(300, 2400, 20, seed=51, zipf=1.1), 128, {"batches": 0},
                         True, 256)
    assert not s["dyn"] and G["cols"] == 1
    check_invariants(e, s)


# ---- balance_pieces -----------------------------------------------------------------------------

def balance_input():
    """One row block; 8 x 400 pieces of lengths 1 + (i * 7) % 16, each of its own column, on one
    workgroup slot per XCD: one item of ~400 pieces (4 phases of NT / G = 128) per XCD."""
    lens = 1 + (np.arange(3200) * 7) % 16
    e = np.repeat(np.arange(3200, dtype=np.uint32), lens)
    geom = np.array([512, 1, 0, 16, 512, 1, 16 * 512, 2048, 1, 0, 0, (80 * 1024 - 8192 - 16) // 4, 1],
                    np.uint32)
    return e, np.array([len(e)], np.uint32), geom, 3200


@pytest.mark.parametrize("kept", [None, [0, 8]])
def test_balance_pieces_permutes_items_without_tiles(kept):
    e, rb_end, geom, NS = balance_input()
    base = {"batches": 0, "item_sched": 0, "item_cap": 0}
    s0 = schedule(e, rb_end, geom, NS, kept=kept, tuning=dict(base, piece_balance=0))
    s1 = schedule(e, rb_end, geom, NS, kept=kept, tuning=dict(base, piece_balance=1))
    assert not s0["dyn"] and not s1["dyn"]
    assert np.array_equal(s0["items"], s1["items"]) and np.array_equal(s0["ends"], s1["ends"])
    check_invariants(e, s0)
    check_invariants(e, s1, longest_first=False)
    npc = s0["ends"].astype(np.int64) - s0["items"][:, 3]
    assert npc.max() >= 257, "no item of >= 3 phases"
    moved = 0
    for it, end in zip(s0["items"], s0["ends"]):
        a, b = s0["pieces"][it[3]:end], s1["pieces"][it[3]:end]
        if it[1] != it[2]:  # kept tiles: untouched
            assert np.array_equal(a, b)
            continue
        key = lambda p: sorted(map(tuple, p))  # noqa: E731
        assert key(a) == key(b), "not a permutation of the item's pieces"
        moved += not np.array_equal(a, b)
    if kept is None:
        assert moved > 0, "piece_balance=1 changed no item"
    else:
        assert (s0["items"][:, 1] != s0["items"][:, 2]).any() and np.array_equal(s0["pieces"], s1["pieces"])


# ---- geometry facts -----------------------------------------------------------------------------

def test_trefethen_20000_geometry():
    """Trefethen_20000 K = 64 on 256 CUs: one 48-row block per workgroup slot (512-thread
    workgroups); the round-2 rule (item_sched 0) keeps the LDS-budget blocks of 576 rows."""
    M, N, rp, ci = synth.trefethen(20000)
    g = dict(zip(GEOM, geometry(256, M, len(ci), N, len(ci), 256)))
    assert g["RB"] == 48 and g["NT"] == 512
    g = dict(zip(GEOM, geometry(256, M, len(ci), N, len(ci), 256,
                                tuning={"item_sched": 0, "item_cap": 0})))
    assert g["RB"] == 576


# ---- thread independence ------------------------------------------------------------------------

def test_result_does_not_depend_on_host_threads():
    # 2,500 blocks of 16 rows: > 2,048 items, so every threaded pass really splits its range
    pat = synth.trefethen(40000)
    one = csr_layout(pat, 64, {"rb_rows": 16}, False, 256, threads=1)[2]
    assert len(one["items"]) >= 2048
    for t in (3, 16):
        many = csr_layout(pat, 64, {"rb_rows": 16}, False, 256, threads=t)[2]
        assert np.array_equal(one["raw"], many["raw"])
    e, rb_end, geom, NS = balance_input()
    tune = {"batches": 0, "piece_balance": 1}
    assert np.array_equal(schedule(e, rb_end, geom, NS, tuning=tune, threads=1)["raw"],
                          schedule(e, rb_end, geom, NS, tuning=tune, threads=7)["raw"])
