"""CPU: the host-only launch decision (csrc/launch_select.cpp) through its device-free debug
exports bsmr_debug_launch_choice, bsmr_debug_rb_form, bsmr_debug_panel_range and
bsmr_debug_col_block_candidate.

The expected values come from the restatement below of the documented rules (DESIGN.md "Launch
selection"), never from the library:

  tile-dominated   4 residual < 16 tiles
  row-block slot   N <= 2^22, layout not colmajor, not tile-dominated unless layout rowblock,
                   N rowBytes < 2^32, rowBytes in {128, 256, 512, 1024, 2048} -> 0 .. 4
  panel-tile       fp16 / bf16, layout auto, ptile != 0, K in {64, 128, 256, 512}, a dense tile, and
                   tile-dominated or ptile = 1
  dense-sampled    fp16 / bf16, layout auto, K % 64 == 0, nnz >= dense_min M N, and K >= 512 or not
                   tile-dominated
  launch           panel-tile, else dense-sampled, else row-block (a slot), else column-major (half
                   for fp16 / bf16, which needs K % 32 == 0); every launch needs K % 16 == 0, K > 0
  row-block form   rb_form_rule below
  column blocks    col_block_rule below
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import bsmr
from bsmr import BF16, F16, F32

_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
PTILE, DENSE, ROWBLOCK, HALF, COLMAJOR = range(5)
OK, INVALID, UNSUPPORTED = 0, 1, 6
KS = (0, 8, 16, 32, 48, 64, 96, 128, 256, 512, 1024, 2048)
LAYOUTS = {"auto": (1, 0), "rowblock": (1, 1), "colmajor": (0, 0)}


def last_error():
    return bsmr.lib().bsmr_last_error().decode()


def _tuning_ptr(tuning):
    return C.byref(bsmr._tuning_struct(tuning or {}))


def launch_choice(facts, layout, K, dtype, tuning=None):
    """(status, kind, slot, rowBytes) of bsmr_debug_launch_choice; facts = (M, N, nnz, nres, tiles)."""
    f = bsmr.lib().bsmr_debug_launch_choice
    f.argtypes = [_u32p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, _u32p]
    out = np.zeros(3, np.uint32)
    st = f(np.array(facts, np.uint32), *LAYOUTS[layout], _tuning_ptr(tuning), K, dtype, out)
    return st, int(out[0]), int(out[1]) - 1, int(out[2])


# ---- the rules, restated --------------------------------------------------------------------------

def tile_dominated(nres, tiles):
    return 4 * nres < 16 * tiles


def slot_rule(facts, layout, K, dtype):
    M, N, nnz, nres, tiles = facts
    if N > 1 << 22 or layout == "colmajor":
        return -1
    if layout != "rowblock" and tile_dominated(nres, tiles):
        return -1
    rby = K * (4 if dtype == F32 else 2)
    if N * rby >= 1 << 32:
        return -1
    return {128: 0, 256: 1, 512: 2, 1024: 3, 2048: 4}.get(rby, -1)


def choice_rule(facts, layout, K, dtype, ptile=-1, dense_min=0.05):
    """(status, kind, slot, rowBytes)."""
    M, N, nnz, nres, tiles = facts
    half = dtype != F32
    slot = slot_rule(facts, layout, K, dtype)
    td = tile_dominated(nres, tiles)
    threshold = float(np.float32(dense_min)) * M * N  # dense_min is a float, the product a double
    if (half and layout == "auto" and ptile != 0 and K in (64, 128, 256, 512) and tiles > 0 and
            (ptile == 1 or td)):
        kind = PTILE
    elif half and layout == "auto" and K % 64 == 0 and nnz >= threshold and (K >= 512 or not td):
        kind = DENSE
    elif slot >= 0:
        kind = ROWBLOCK
    else:
        kind = HALF if half else COLMAJOR
    status = OK
    if K == 0 or K % 16 or (kind == HALF and K % 32):
        status = UNSUPPORTED
    return status, kind, slot, K * (2 if half else 4)


# facts (M, N, nnz, nres, tiles): a residual-dominated plan, no dense tile, the tile-dominated
# boundary (16 tiles = 1600 against 4 nres = 1596 / 1600 / 1604), N around 2^22, N rowBytes around
# 2^32 for 1 KiB and 2 KiB rows (one row below, exactly at)
FACTS = {
    "residual": (1000, 4000, 30000, 20000, 70),
    "no_tiles": (1000, 4000, 30000, 30000, 0),
    "td_below": (512, 512, 26000, 399, 100),
    "td_equal": (512, 512, 26001, 400, 100),
    "td_above": (512, 512, 26002, 401, 100),
    "tiles_only": (512, 512, 41984, 0, 164),
    "N_2p22": (1000, 1 << 22, 30000, 20000, 70),
    "N_2p22_plus_1": (1000, (1 << 22) + 1, 30000, 20000, 70),
    "B_4GiB_1k_below": (1000, (1 << 22) - 1, 30000, 20000, 70),
    "B_4GiB_2k_below": (1000, (1 << 21) - 1, 30000, 20000, 70),
    "B_4GiB_2k_at": (1000, 1 << 21, 30000, 20000, 70),
}


@pytest.mark.parametrize("name", sorted(FACTS))
def test_launch_choice_follows_the_rules(name):
    facts = FACTS[name]
    for layout, dtype, K, ptile in itertools.product(LAYOUTS, (F32, F16, BF16), KS, (-1, 0, 1)):
        tuning = {} if ptile < 0 else {"ptile": ptile}
        got = launch_choice(facts, layout, K, dtype, tuning)
        want = choice_rule(facts, layout, K, dtype, ptile)
        assert got == want, (name, layout, dtype, K, ptile, got, want)


def test_the_boundaries_fall_where_the_rules_put_them():
    """The sweep above compares against the restated rules; here the outcomes at the boundaries are
    spelled out, so that a restatement wrong in the same way as the library would still fail."""
    def kind_slot(facts, layout, K, dtype, tuning=None):
        st, kind, slot, _ = launch_choice(facts, layout, K, dtype, tuning)
        assert st == OK, last_error()
        return kind, slot

    # tile-dominated is strict: 4 nres < 16 tiles
    assert kind_slot(FACTS["td_below"], "auto", 128, F32) == (COLMAJOR, -1)
    assert kind_slot(FACTS["td_equal"], "auto", 128, F32) == (ROWBLOCK, 2)
    assert kind_slot(FACTS["td_above"], "auto", 128, F32) == (ROWBLOCK, 2)
    assert kind_slot(FACTS["td_below"], "rowblock", 128, F32) == (ROWBLOCK, 2)
    assert kind_slot(FACTS["td_below"], "auto", 128, BF16) == (PTILE, -1)
    assert kind_slot(FACTS["td_equal"], "auto", 128, BF16)[0] != PTILE
    assert kind_slot(FACTS["td_equal"], "auto", 128, BF16, {"ptile": 1}) == (PTILE, 1)  # the slot stays
    assert kind_slot(FACTS["td_below"], "auto", 128, BF16, {"ptile": 0}) == (HALF, -1)
    assert kind_slot(FACTS["no_tiles"], "auto", 128, BF16, {"ptile": 1}) == (ROWBLOCK, 1)
    # both the panel-tile and the dense-sampled rule hold (16 % dense, K = 512): panel-tile first
    assert kind_slot(FACTS["tiles_only"], "auto", 512, BF16) == (PTILE, -1)
    assert kind_slot(FACTS["tiles_only"], "auto", 512, BF16, {"ptile": 0}) == (DENSE, -1)
    assert kind_slot(FACTS["tiles_only"], "auto", 256, BF16, {"ptile": 0}) == (HALF, -1)  # K < 512
    # N <= 2^22 and B < 4 GiB
    assert kind_slot(FACTS["N_2p22"], "auto", 128, F32) == (ROWBLOCK, 2)
    assert kind_slot(FACTS["N_2p22_plus_1"], "auto", 128, F32) == (COLMAJOR, -1)
    assert kind_slot(FACTS["B_4GiB_1k_below"], "auto", 256, F32) == (ROWBLOCK, 3)
    assert kind_slot(FACTS["N_2p22"], "auto", 256, F32) == (COLMAJOR, -1)  # 2^22 x 1 KiB = 2^32
    assert kind_slot(FACTS["B_4GiB_1k_below"], "auto", 512, F16) == (ROWBLOCK, 3)
    assert kind_slot(FACTS["N_2p22"], "auto", 512, F16) == (HALF, -1)
    assert kind_slot(FACTS["B_4GiB_2k_below"], "auto", 512, F32) == (ROWBLOCK, 4)
    assert kind_slot(FACTS["B_4GiB_2k_at"], "auto", 512, F32) == (COLMAJOR, -1)
    # layouts
    assert kind_slot(FACTS["residual"], "colmajor", 128, F32) == (COLMAJOR, -1)
    assert kind_slot(FACTS["residual"], "colmajor", 128, F16) == (HALF, -1)
    assert kind_slot(FACTS["residual"], "auto", 192, F32) == (COLMAJOR, -1)  # 768-byte rows: no slot


@pytest.mark.parametrize("dense_min,M,N,edge", [(None, 2048, 2048, 209716), (0.25, 512, 512, 65536),
                                                (0.05, 1000, 3000, 150001)])
def test_dense_threshold(dense_min, M, N, edge):
    """nnz one below and at dense_min M N (0.05f is a little over 0.05: 209715.2.. and 150000.001..
    round up; 0.25 is exact), on a residual-dominated plan, and under each layout."""
    tuning = {} if dense_min is None else {"dense_min": dense_min}
    dm = 0.05 if dense_min is None else dense_min
    for nnz, dense in ((edge - 1, False), (edge, True)):
        facts = (M, N, nnz, nnz, 0)
        for layout, dtype, K in itertools.product(LAYOUTS, (F32, F16, BF16), KS):
            got = launch_choice(facts, layout, K, dtype, tuning)
            assert got == choice_rule(facts, layout, K, dtype, dense_min=dm), (nnz, layout, dtype, K)
        assert (launch_choice(facts, "auto", 128, BF16, tuning)[1] == DENSE) == dense
        assert launch_choice(facts, "auto", 128, F32, tuning)[1] == ROWBLOCK
        assert launch_choice(facts, "rowblock", 128, BF16, tuning)[1] == ROWBLOCK
        assert launch_choice(facts, "auto", 96, BF16, tuning)[1] == HALF  # K % 64


def test_k_and_dtype_rules_and_their_texts():
    who = "bsmr_debug_launch_choice"
    for dtype in (F32, F16, BF16):
        for K in (0, 8, 24):
            assert launch_choice(FACTS["residual"], "auto", K, dtype)[0] == UNSUPPORTED
            assert last_error() == who + ": K must be a positive multiple of 16"
    assert launch_choice(FACTS["residual"], "auto", 64, 3)[0] == UNSUPPORTED
    assert last_error() == who + ": dtype must be BSMR_F32, BSMR_F16 or BSMR_BF16"
    for K in (16, 48, 80):  # the half column-major launch
        assert launch_choice(FACTS["residual"], "auto", K, F16) == (UNSUPPORTED, HALF, -1, 2 * K)
        assert last_error() == who + ": fp16/bf16 inputs need K to be a positive multiple of 32"
        assert launch_choice(FACTS["residual"], "auto", K, F32)[0] == OK
    assert launch_choice(FACTS["residual"], "auto", 96, F16) == (OK, HALF, -1, 192)
    assert launch_choice(FACTS["residual"], "auto", 64, F16) == (OK, ROWBLOCK, 0, 128)  # a slot: any K % 16


# ---- the form of a row-block launch ---------------------------------------------------------------

FORM = ("stageNt", "lateB", "pairs", "lite", "dyn", "NT", "grid", "ldsBytes", "stageBlocks")
LFACTS = ("rowBytes", "NT", "nItems", "nTilesKept", "outLds", "outRuns", "dynBatches")


def rb_form(layout, tuning=None, mode=3):
    f = bsmr.lib().bsmr_debug_rb_form
    f.argtypes = [_u32p, C.c_void_p, C.c_uint32, _u32p]
    out = np.zeros(len(FORM), np.uint32)
    assert f(np.array([layout[k] for k in LFACTS], np.uint32), _tuning_ptr(tuning), mode, out) == 0
    return dict(zip(FORM, (int(v) for v in out)))


def rb_form_rule(L, tuning=None, mode=3):
    t = dict(stage_nt=-1, late_b=-1, pair_min_items=4096, diag=0)
    t.update(tuning or {})
    stage_nt = t["stage_nt"] == 1  # (auto stages with the default policy)
    late_b = t["late_b"] != 0
    pairs = (mode == 3 and L["outRuns"] and L["outLds"] and L["rowBytes"] >= 512 and
             L["nItems"] >= t["pair_min_items"] and L["nTilesKept"] == 0 and L["nItems"] % 16 == 0 and
             not stage_nt and late_b and not t["diag"] & (8 | 32 | 64 | 128 | 16384))
    lite = (mode == 3 and L["nTilesKept"] == 0 and not L["outLds"] and not stage_nt and late_b and
            t["diag"] == 0)
    return dict(stageNt=int(stage_nt), lateB=int(late_b), pairs=int(bool(pairs)), lite=int(bool(lite)),
                dyn=L["dynBatches"], NT=L["NT"], grid=L["nItems"] // 2 if pairs else L["nItems"],
                ldsBytes=(160 if L["NT"] == 1024 else 80) * 1024,
                stageBlocks=(159 if L["NT"] == 1024 else 79) if t["diag"] & 2097152 else 0)


PAIRING = dict(rowBytes=512, NT=1024, nItems=4096, nTilesKept=0, outLds=122880, outRuns=1, dynBatches=0)
LITE = dict(rowBytes=512, NT=512, nItems=1000, nTilesKept=0, outLds=0, outRuns=0, dynBatches=0)

PAIR_FLIPS = {
    "outRuns": (dict(outRuns=0), {}, 3), "outLds": (dict(outLds=0), {}, 3),
    "rowBytes": (dict(rowBytes=256), {}, 3), "few_items": (dict(nItems=4080), {}, 3),
    "items_mod_16": (dict(nItems=4104), {}, 3), "kept_tile": (dict(nTilesKept=1), {}, 3),
    "stage_nt": ({}, {"stage_nt": 1}, 3), "late_b": ({}, {"late_b": 0}, 3),
    "mode_1": ({}, {}, 1), "mode_2": ({}, {}, 2),
    **{f"diag_{b}": ({}, {"diag": b}, 3) for b in (8, 32, 64, 128, 16384)},
}
LITE_FLIPS = {
    "mode_1": ({}, {}, 1), "mode_2": ({}, {}, 2), "kept_tile": (dict(nTilesKept=1), {}, 3),
    "outLds": (dict(outLds=81920), {}, 3), "stage_nt": ({}, {"stage_nt": 1}, 3),
    "late_b": ({}, {"late_b": 0}, 3), "diag_1": ({}, {"diag": 1}, 3),
    "diag_keep_full": ({}, {"diag": 33554432}, 3),
}


def test_the_two_starting_layouts():
    p = rb_form(PAIRING)
    assert p == rb_form_rule(PAIRING)
    assert (p["pairs"], p["lite"], p["grid"], p["NT"], p["ldsBytes"]) == (1, 0, 2048, 1024, 160 * 1024)
    assert (p["stageNt"], p["lateB"], p["dyn"], p["stageBlocks"]) == (0, 1, 0, 0)
    lite = rb_form(LITE)
    assert lite == rb_form_rule(LITE)
    assert (lite["pairs"], lite["lite"], lite["grid"], lite["NT"], lite["ldsBytes"]) == (0, 1, 1000, 512, 80 * 1024)
    # at the thresholds: 512-byte rows, pair_min_items items
    assert rb_form(dict(PAIRING, nItems=16), {"pair_min_items": 16})["pairs"] == 1
    assert rb_form(dict(PAIRING, nItems=16), {"pair_min_items": 17})["pairs"] == 0
    assert rb_form(dict(PAIRING, rowBytes=2048))["pairs"] == 1


@pytest.mark.parametrize("name", sorted(PAIR_FLIPS))
def test_each_pair_condition_alone_clears_pairs(name):
    change, tuning, mode = PAIR_FLIPS[name]
    L = dict(PAIRING, **change)
    got = rb_form(L, tuning, mode)
    assert got == rb_form_rule(L, tuning, mode), name
    assert got["pairs"] == 0 and got["grid"] == L["nItems"]
    # nothing else moves, but what the flipped input itself sets: direct stores make the launch lite
    base = rb_form(PAIRING)
    moved = {k for k in FORM if got[k] != base[k]} - {"pairs", "grid"}
    assert moved == {"outLds": {"lite"}, "stage_nt": {"stageNt"}, "late_b": {"lateB"}}.get(name, set()), moved


@pytest.mark.parametrize("name", sorted(LITE_FLIPS))
def test_each_lite_condition_alone_clears_lite(name):
    change, tuning, mode = LITE_FLIPS[name]
    L = dict(LITE, **change)
    got = rb_form(L, tuning, mode)
    assert got == rb_form_rule(L, tuning, mode), name
    assert got["lite"] == 0
    base = rb_form(LITE)
    moved = {k for k in FORM if got[k] != base[k]} - {"lite"}
    assert moved == {"stage_nt": {"stageNt"}, "late_b": {"lateB"}}.get(name, set()), moved


def test_launch_configuration():
    for nt, lds, blocks in ((512, 80 * 1024, 79), (1024, 160 * 1024, 159)):
        for base in (PAIRING, LITE):
            L = dict(base, NT=nt)
            f = rb_form(L)
            assert (f["NT"], f["ldsBytes"], f["stageBlocks"]) == (nt, lds, 0)  # 0: the image's own blocks
            g = rb_form(L, {"diag": 2097152})
            assert g == rb_form_rule(L, {"diag": 2097152})
            assert (g["stageBlocks"], g["ldsBytes"], g["lite"]) == (blocks, lds, 0)
            assert g["pairs"] == f["pairs"]  # not one of the bits that unpair
    assert rb_form(dict(LITE, dynBatches=1))["dyn"] == 1
    assert rb_form(dict(PAIRING, dynBatches=1)) == dict(rb_form(PAIRING), dyn=1)
    # auto nt staging (stage_nt = -1) is off for staged and unstaged output alike
    assert rb_form(PAIRING, {"stage_nt": -1})["stageNt"] == 0 and rb_form(LITE, {"stage_nt": 0})["stageNt"] == 0


# ---- the panel-range rules of the four panel entry points ------------------------------------------

def panel_range(who, p0, p1, P, slot, dtype, local):
    f = bsmr.lib().bsmr_debug_panel_range
    f.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int]
    return f(who.encode(), p0, p1, P, slot, dtype, int(local))


LOCAL_TEXT = {  # the launch speaks for itself, the others name it
    "bsmr_sddmm_panels_local": ": needs the row-block launch (rows of 128 B .. 2 KiB)",
    "bsmr_plan_prepare_panels": ": bsmr_sddmm_panels_local needs the row-block launch (rows of 128 B .. 2 KiB)",
    "bsmr_plan_panels_prepared": ": bsmr_sddmm_panels_local needs the row-block launch (rows of 128 B .. 2 KiB)",
}


@pytest.mark.parametrize("who", ["bsmr_sddmm_panels", "bsmr_sddmm_panels_local", "bsmr_plan_prepare_panels",
                                 "bsmr_plan_panels_prepared"])
def test_panel_range_codes_and_texts(who):
    P = 40
    for dtype, slot, local in itertools.product((F32, F16, BF16), (-1, 0, 4), (False, True)):
        for p0, p1 in ((5, 4), (0, P + 1), (P + 1, P + 1), (P + 2, P + 1)):  # a bad range, whatever else
            assert panel_range(who, p0, p1, P, slot, dtype, local) == INVALID
            assert last_error() == who + ": bad panel range"
        for p0 in (0, 7, P):  # an empty range is fine, with or without a slot
            assert panel_range(who, p0, p0, P, slot, dtype, local) == OK
        assert panel_range(who, 0, P, P, 2, dtype, local) == OK
    for dtype in (F32, F16, BF16):
        if who in LOCAL_TEXT:  # local A rows without a row-block slot
            assert panel_range(who, 3, 9, P, -1, dtype, True) == UNSUPPORTED
            assert last_error() == who + LOCAL_TEXT[who]
    for dtype in (F16, BF16):  # half operands without a slot
        assert panel_range(who, 3, 9, P, -1, dtype, False) == UNSUPPORTED
        assert last_error() == who + ": fp16/bf16 panel ranges need the row-block layout (half K in 128..1024)"
    assert panel_range(who, 3, 9, P, -1, F32, False) == OK  # fp32: the panel-major lists


# ---- the column-block candidate ---------------------------------------------------------------------

def col_block_candidate(M, N, col_blocks, row_bytes):
    f = bsmr.lib().bsmr_debug_col_block_candidate
    f.argtypes = [_u32p, C.c_int, C.c_uint32]
    f.restype = C.c_int
    return f(np.array([M, N, 0, 0, 0], np.uint32), col_blocks, row_bytes)


def col_block_rule(M, N, col_blocks, row_bytes):
    """The column-block launch swaps the operands: it gathers A rows through the metadata's 22-bit
    column field and load_bcol's 32-bit byte offset, so the candidate (col_blocks = 1, or 2 on a
    wide pattern) exists only when M <= 2^22 and M rowBytes < 2^32."""
    asked = col_blocks == 1 or (col_blocks == 2 and N >= 2 * M)
    return int(asked and M <= 1 << 22 and M * row_bytes < 1 << 32)


def test_col_block_candidate_follows_the_rule():
    for M, N, cb, rby in itertools.product(
            (1, 1500, (1 << 21) - 1, 1 << 21, (1 << 21) + 64, (1 << 22) - 1, 1 << 22, (1 << 22) + 1),
            (192, 2999, 3000, 1 << 22), (-1, 0, 1, 2, 3), (128, 256, 512, 1024, 2048)):
        assert col_block_candidate(M, N, cb, rby) == col_block_rule(M, N, cb, rby), (M, N, cb, rby)


def test_col_block_candidate_boundaries():
    """Spelled out: A of 2^21 - 1, 2^21 and 2^21 + 64 rows of 2 KiB (one row under 4 GiB, exactly
    4 GiB, past it) and of 2^22 and 2^22 + 1 rows of 128 B (the 22-bit row field), under
    col_blocks = 1; a taller A never gets column blocks, whatever is asked."""
    assert col_block_candidate((1 << 21) - 1, 192, 1, 2048) == 1
    assert col_block_candidate(1 << 21, 192, 1, 2048) == 0
    assert col_block_candidate((1 << 21) + 64, 192, 1, 2048) == 0
    assert col_block_candidate((1 << 21) + 64, 192, 1, 1024) == 1  # 1 KiB rows: 2 GiB + 64 KiB
    assert col_block_candidate(1 << 22, 192, 1, 128) == 1
    assert col_block_candidate((1 << 22) + 1, 192, 1, 128) == 0
    assert col_block_candidate(1 << 22, 192, 1, 1024) == 0  # 2^22 x 1 KiB = 2^32
    # rule 2 asks for N >= 2 M first; what rb_slot admits then always fits
    assert col_block_candidate(1500, 3000, 2, 128) == 1
    assert col_block_candidate(1500, 2999, 2, 128) == 0
    assert col_block_candidate(1500, 3000, 0, 128) == 0 and col_block_candidate(1500, 3000, -1, 128) == 0
