"""The frozen row-block layouts: the case table, the layout words and their digest.

tools/rb_layout_digest.py records one digest per case into tests/golden/mi355x_rb_layout_digests.json;
test_gpu_rb_layout_frozen.py (device plans) and test_rb_schedule_cpu.py (the host-only scheduler)
compare against that file. The digest is the SHA-256 of little-endian u32 words:
{RB, NT, rowBytes, nItems, nPieces}, the items (4 u32 each: row block, tile begin, tile end, piece
begin), the item ends, the pieces (2 u32 each) — what bsmr_debug_rb_items and bsmr_debug_rb_pieces
return for the whole plan's layout of (K, dtype).
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np

import bsmr
from bsmr import F32, Plan, synth
from test_gpu_plan_check import LAYOUTS, WIDE, ZIPF

FREE = 288 * 1024 ** 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "mi355x_rb_layout_digests.json")
NOT_ROWBLOCK = ("colmajor", "colmajor_half", "dense_sampled", "ptile_over_dense")
# LAYOUTS rows whose plans are cases of the table below already (zipf/piece_balance,
# wide_staged/piece_balance_k256)
SAME_PLAN = ("piece_balance", "piece_balance_staged_1k")

TREF3000 = lambda: synth.trefethen(3000)  # noqa: E731
COLS_LOCAL = lambda: synth.random_rows(500, 4000, 24, seed=31, zipf=1.2)  # noqa: E731


def _cases():
    # name: (pattern, K, dtype, plan kwargs), as LAYOUTS
    c = {"plan_check/" + k: v for k, v in LAYOUTS.items() if k not in NOT_ROWBLOCK + SAME_PLAN}
    for name, t in [("round2_lists", {"item_sched": 0, "item_cap": 0}),
                    ("item_cap_1", {"item_cap": 1.0}),
                    ("piece_max_4", {"piece_max": 4}),
                    ("rb_rows_64", {"rb_rows": 64}),
                    ("piece_balance", {"piece_balance": 1})]:
        c["zipf/" + name] = (ZIPF, 128, F32, {"tuning": t})
    for name, K, t in [("l2_range_256", 128, {"l2_range_kb": 256}),
                       ("piece_balance_k128", 128, {"piece_balance": 1}),
                       ("piece_balance_k256", 256, {"piece_balance": 1}),
                       ("piece_balance_k512", 512, {"piece_balance": 1})]:
        c["wide_staged/" + name] = (WIDE, K, F32, {"tuning": dict({"out_staged": 1}, **t)})
    c["wide/col_blocks"] = (WIDE, 128, F32, {"tuning": {"col_blocks": 1}})
    c["cols_local/col_blocks"] = (COLS_LOCAL, 128, F32, {"tuning": {"col_blocks": 1}})
    c["trefethen3000/orig_not_contig"] = (TREF3000, 64, F32,
                                          {"tuning": {"orig_rows": 1, "orig_contig": 0}})
    c["mycielskian11/rowblock"] = (lambda: synth.mycielskian(11), 128, F32, {"layout": "rowblock"})
    # unsplit blocks dealt to the shortest list (no list scheduling, not contiguous)
    c["trefethen3000/orig_round2_rb16"] = (
        TREF3000, 64, F32, {"tuning": {"orig_rows": 1, "orig_contig": 0, "item_sched": 0, "item_cap": 0,
                                       "rb_rows": 16}})
    # 512-byte rows with many pieces per row-group: dynamic batches chosen by the auto rule
    c["mycielskian14/rowblock"] = (lambda: synth.mycielskian(14), 128, F32, {"layout": "rowblock"})
    return c


CASES = _cases()


def layout_words(RB, NT, row_bytes, items, item_end, pieces):
    """The digest's u32 words from the header values, items (n x 4), item ends (n), pieces (p x 2)."""
    items = np.asarray(items, np.uint32).reshape(-1, 4)
    pieces = np.asarray(pieces, np.uint32).reshape(-1, 2)
    item_end = np.asarray(item_end, np.uint32).reshape(-1)
    assert len(item_end) == len(items)
    head = np.array([RB, NT, row_bytes, len(items), len(pieces)], np.uint32)
    return np.concatenate([head, items.reshape(-1), item_end, pieces.reshape(-1)])


def digest(words):
    return hashlib.sha256(np.ascontiguousarray(words, "<u4").tobytes()).hexdigest()


def _export(fn, plan, K, dtype):
    f = getattr(bsmr.lib(), fn)
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    n = C.c_uint64()
    assert f(plan.h, K, dtype, None, C.byref(n)) == 0, bsmr.lib().bsmr_last_error()
    buf = np.zeros(n.value, np.uint32)
    assert f(plan.h, K, dtype, buf.ctypes.data, C.byref(n)) == 0, bsmr.lib().bsmr_last_error()
    return buf


def plan_layout_words(plan, K, dtype):
    """The whole-plan row-block layout of (K, dtype) of a device plan, as digest words."""
    hdr = _export("bsmr_debug_rb_items", plan, K, dtype)
    assert len(hdr) >= 4, "no row-block layout for this (K, dtype)"
    buf = _export("bsmr_debug_rb_pieces", plan, K, dtype)
    n, p = int(buf[0]), int(buf[1])
    assert len(buf) == 2 + 5 * n + 2 * p and int(hdr[2]) == n
    return layout_words(hdr[0], hdr[1], hdr[3], buf[2:2 + 4 * n], buf[2 + 4 * n:2 + 5 * n],
                        buf[2 + 5 * n:])


def case_plan(name):
    pat, K, dtype, kw = CASES[name]
    M, N, rp, ci = pat()
    return Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, **kw), K, dtype


def case_digest(name):
    plan, K, dtype = case_plan(name)
    return digest(plan_layout_words(plan, K, dtype))


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
