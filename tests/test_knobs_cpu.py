"""CPU: the plan's tuning unit (csrc/knobs.cpp): bsmr_tuning and bsmr_plan_options onto Knobs.

tests/knobs_main.cpp compiles csrc/knobs.cpp alone, with a host compiler, AddressSanitizer and
UBSan and no HIP include path: that it builds shows the unit is host-only. Nothing loaded into
Python is sanitized.

`apply`: rows of (the 26 fields of bsmr_tuning, layout, lds_budget_kb, cluster_batch) go through
apply_options and come back as every member of Knobs. What each row must give is written out
below, by hand, from the rules the plan has always applied: the defaults, every field alone at a
representative value, every clamp on both sides, the three layouts, the LDS budget's bounds with
the exact error text, and cluster_batch.

`env`: the program itself sets each field's BSMR_<FIELD> variable and checks bsmr_tuning_default
and bsmr_tuning_from_env on all 26 fields (atoi, atof and the tri-state rule).
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sddmm-gpu_amd", "csrc")

# bsmr_tuning in the order of include/bsmr.h
FIELDS = ["diag", "tile_min_f32", "tile_min_half", "piece_max", "piece_weight", "shard_piece_weight", "dense_min",
          "orig_rows", "orig_contig", "dense_ks", "dense_ns", "out_staged", "l2_range_kb", "stage_nt", "rb_rows",
          "late_b", "item_cap", "item_sched", "out_packed", "cluster_filter", "pair_min_items", "batches", "ptile",
          "ptile_tpi", "piece_balance", "col_blocks"]
AUTO = dict({f: -1 for f in FIELDS}, diag=0)
AUTO_LAYOUT, ROWBLOCK, COLMAJOR = 0, 1, 2

# what a plan created without options or tuning holds
DEFAULTS = dict(
    use_rowblock=1, force_rowblock=0, rb_lds_kb=144, rb_lds_user=0, rb_lds_kb_staged=120, l2_range_kb_staged=4096,
    diag=0, l2_range_kb=2048, l2_range_user=0, piece_max=16, piece_weight=4.0, shard_piece_weight=4.0,
    out_staged=-1, out_packed=-1, stage_nt=-1, rb_rows_force=-1, late_b=-1, item_cap=-1.0, item_cost_cuts=1,
    item_lpt=1, item_fixed=1024.0, small_sparse_rb=1, out_staged_min=8 << 20, dense_min=0.05, cluster_batch=16384,
    cluster_filter=-1, filter_min_rows=32768, pair_min_items=4096, batches=-1, batch_min_phases=2.0,
    piece_balance=0, orig_rows=-1, col_blocks=0, orig_contig=1, tile_min_f32=257, tile_min_half=128, dense_ks=0,
    dense_ns=2, ptile_mode=-1, ptile_tpi=0)
BAD = "bsmr_plan: bad layout or lds_budget_kb"
ITEM_SCHED_OFF = dict(item_cost_cuts=0, item_lpt=0, small_sparse_rb=0)

# (name, tuning fields, layout, lds_budget_kb, cluster_batch, status, the Knobs members that differ
# from DEFAULTS, message)
CASES = [
    ("defaults", {}, AUTO_LAYOUT, 0, 0, 0, {}, ""),
    # each field alone
    ("diag", {"diag": 2097152 + 32}, 0, 0, 0, 0, {"diag": 2097152 + 32}, ""),
    ("tile_min_f32", {"tile_min_f32": 100}, 0, 0, 0, 0, {"tile_min_f32": 100}, ""),
    ("tile_min_f32_0", {"tile_min_f32": 0}, 0, 0, 0, 0, {"tile_min_f32": 0}, ""),
    ("tile_min_half", {"tile_min_half": 64}, 0, 0, 0, 0, {"tile_min_half": 64}, ""),
    ("piece_max", {"piece_max": 8}, 0, 0, 0, 0, {"piece_max": 8}, ""),
    ("piece_max_low", {"piece_max": 0}, 0, 0, 0, 0, {"piece_max": 1}, ""),
    ("piece_max_high", {"piece_max": 99}, 0, 0, 0, 0, {"piece_max": 16}, ""),
    ("piece_weight", {"piece_weight": 2.5}, 0, 0, 0, 0, {"piece_weight": 2.5}, ""),
    ("piece_weight_0", {"piece_weight": 0}, 0, 0, 0, 0, {"piece_weight": 0.0}, ""),
    ("shard_piece_weight", {"shard_piece_weight": 8}, 0, 0, 0, 0, {"shard_piece_weight": 8.0}, ""),
    ("dense_min", {"dense_min": 0.25}, 0, 0, 0, 0, {"dense_min": 0.25}, ""),
    ("orig_rows_0", {"orig_rows": 0}, 0, 0, 0, 0, {"orig_rows": 0}, ""),
    ("orig_rows_1", {"orig_rows": 1}, 0, 0, 0, 0, {"orig_rows": 1}, ""),
    ("orig_contig", {"orig_contig": 0}, 0, 0, 0, 0, {"orig_contig": 0}, ""),
    ("orig_contig_as_given", {"orig_contig": 3}, 0, 0, 0, 0, {"orig_contig": 3}, ""),
    ("dense_ks", {"dense_ks": 2}, 0, 0, 0, 0, {"dense_ks": 2}, ""),
    ("dense_ns", {"dense_ns": 5}, 0, 0, 0, 0, {"dense_ns": 5}, ""),
    ("out_staged_0", {"out_staged": 0}, 0, 0, 0, 0, {"out_staged": 0}, ""),
    ("out_staged_1", {"out_staged": 1}, 0, 0, 0, 0, {"out_staged": 1}, ""),
    ("l2_range_kb", {"l2_range_kb": 1024}, 0, 0, 0, 0, {"l2_range_kb": 1024, "l2_range_user": 1}, ""),
    ("l2_range_kb_low", {"l2_range_kb": 10}, 0, 0, 0, 0, {"l2_range_kb": 64, "l2_range_user": 1}, ""),
    ("l2_range_kb_default_given", {"l2_range_kb": 2048}, 0, 0, 0, 0, {"l2_range_user": 1}, ""),
    ("stage_nt_0", {"stage_nt": 0}, 0, 0, 0, 0, {"stage_nt": 0}, ""),
    ("stage_nt_1", {"stage_nt": 1}, 0, 0, 0, 0, {"stage_nt": 1}, ""),
    ("rb_rows", {"rb_rows": 48}, 0, 0, 0, 0, {"rb_rows_force": 48}, ""),
    ("rb_rows_0", {"rb_rows": 0}, 0, 0, 0, 0, {}, ""),
    ("late_b_0", {"late_b": 0}, 0, 0, 0, 0, {"late_b": 0}, ""),
    ("late_b_as_given", {"late_b": 2}, 0, 0, 0, 0, {"late_b": 2}, ""),
    ("item_cap", {"item_cap": 1.5}, 0, 0, 0, 0, {"item_cap": 1.5}, ""),
    ("item_cap_0", {"item_cap": 0}, 0, 0, 0, 0, {"item_cap": 0.0}, ""),
    ("item_sched_0", {"item_sched": 0}, 0, 0, 0, 0, ITEM_SCHED_OFF, ""),
    ("item_sched_1", {"item_sched": 1}, 0, 0, 0, 0, {}, ""),
    ("out_packed_0", {"out_packed": 0}, 0, 0, 0, 0, {"out_packed": 0}, ""),
    ("out_packed_normalised", {"out_packed": 7}, 0, 0, 0, 0, {"out_packed": 1}, ""),
    ("cluster_filter_0", {"cluster_filter": 0}, 0, 0, 0, 0, {"cluster_filter": 0}, ""),
    ("cluster_filter_1", {"cluster_filter": 1}, 0, 0, 0, 0, {"cluster_filter": 1}, ""),
    ("pair_min_items", {"pair_min_items": 16}, 0, 0, 0, 0, {"pair_min_items": 16}, ""),
    ("pair_min_items_0", {"pair_min_items": 0}, 0, 0, 0, 0, {"pair_min_items": 0}, ""),
    ("batches_0", {"batches": 0}, 0, 0, 0, 0, {"batches": 0}, ""),
    ("batches_1", {"batches": 1}, 0, 0, 0, 0, {"batches": 1}, ""),
    ("ptile_0", {"ptile": 0}, 0, 0, 0, 0, {"ptile_mode": 0}, ""),
    ("ptile_1", {"ptile": 1}, 0, 0, 0, 0, {"ptile_mode": 1}, ""),
    ("ptile_tpi", {"ptile_tpi": 4}, 0, 0, 0, 0, {"ptile_tpi": 4}, ""),
    ("ptile_tpi_high", {"ptile_tpi": 100}, 0, 0, 0, 0, {"ptile_tpi": 64}, ""),
    ("piece_balance_1", {"piece_balance": 1}, 0, 0, 0, 0, {"piece_balance": 1}, ""),
    ("piece_balance_0", {"piece_balance": 0}, 0, 0, 0, 0, {}, ""),
    ("col_blocks_1", {"col_blocks": 1}, 0, 0, 0, 0, {"col_blocks": 1}, ""),
    ("col_blocks_2", {"col_blocks": 2}, 0, 0, 0, 0, {"col_blocks": 2}, ""),
    ("col_blocks_high", {"col_blocks": 5}, 0, 0, 0, 0, {"col_blocks": 2}, ""),
    # every "0/1" knob normalised with != 0
    ("switches_normalised", {f: 7 for f in ("orig_rows", "out_staged", "out_packed", "stage_nt", "item_sched",
                                            "cluster_filter", "batches", "ptile", "piece_balance")}, 0, 0, 0, 0,
     dict(orig_rows=1, out_staged=1, out_packed=1, stage_nt=1, cluster_filter=1, batches=1, ptile_mode=1,
          piece_balance=1), ""),
    # the options
    ("layout_rowblock", {}, ROWBLOCK, 0, 0, 0, {"force_rowblock": 1}, ""),
    ("layout_colmajor", {}, COLMAJOR, 0, 0, 0, {"use_rowblock": 0}, ""),
    ("layout_low", {}, -1, 0, 0, 1, None, BAD),
    ("layout_high", {}, 3, 0, 0, 1, None, BAD),
    ("lds_15", {}, 0, 15, 0, 1, None, BAD),
    ("lds_16", {}, 0, 16, 0, 0, {"rb_lds_kb": 16, "rb_lds_user": 1}, ""),
    ("lds_160", {}, 0, 160, 0, 0, {"rb_lds_kb": 160, "rb_lds_user": 1}, ""),
    ("lds_161", {}, 0, 161, 0, 1, None, BAD),
    ("lds_default_given", {}, 0, 144, 0, 0, {"rb_lds_user": 1}, ""),
    ("cluster_batch", {}, 0, 0, 512, 0, {"cluster_batch": 512}, ""),
    ("cluster_batch_0", {}, 0, 0, 0, 0, {}, ""),
    ("together", {"item_sched": 0, "item_cap": 0, "l2_range_kb": 4096, "col_blocks": 2, "diag": 8}, ROWBLOCK, 96,
     4096, 0, dict(ITEM_SCHED_OFF, item_cap=0.0, l2_range_kb=4096, l2_range_user=1, col_blocks=2, diag=8,
                   force_rowblock=1, rb_lds_kb=96, rb_lds_user=1, cluster_batch=4096), ""),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("knobs_asan")
    exe = str(d / "knobs_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "knobs_main.cpp"),
           os.path.join(CSRC, "knobs.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime (the linker's message) is a skip; any other error fails
        if re.search(r"cannot find -l(asan|ubsan)\b|cannot find \S*lib(asan|ubsan)\S*", r.stderr):
            pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
        raise AssertionError(r.stderr)
    return exe, d


@pytest.fixture(scope="module")
def applied(driver):
    """Every case through the program once: name -> (status, {member: value}, message)."""
    exe, d = driver
    path = str(d / "rows.txt")
    with open(path, "w") as f:
        for _, tuning, layout, lds, batch, *_ in CASES:
            t = dict(AUTO, **tuning)
            f.write(" ".join(repr(t[k]) for k in FIELDS) + f" {layout} {lds} {batch}\n")
    r = subprocess.run([exe, "apply", path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES)
    out = {}
    for case, line in zip(CASES, lines):
        words, msg = line.split(" | ") if not line.endswith(" | ") else (line[:-3], "")
        w = words.split()
        assert w[0] == "code"
        out[case[0]] = (int(w[1]), {k: float(v) for k, v in zip(w[2::2], w[3::2])}, msg)
    return out


def test_the_cases_name_every_field_and_member():
    assert len(FIELDS) == 26 and len(DEFAULTS) == 40
    assert set(FIELDS) == set().union(*(c[1] for c in CASES))
    changed = set().union(*(c[6] for c in CASES if c[6]))
    # members no field or option reaches keep their default in every case
    assert set(DEFAULTS) - changed == {"rb_lds_kb_staged", "l2_range_kb_staged", "item_fixed", "out_staged_min",
                                       "filter_min_rows", "batch_min_phases"}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_apply(applied, case):
    name, _, _, _, _, status, differ, message = case
    got_status, got, got_message = applied[name]
    assert (got_status, got_message) == (status, message)
    if status:
        return  # rejected: the plan is not created
    assert list(got) == list(DEFAULTS), "every member, in the order of Knobs"
    # exact: every value of the cases is a binary fraction; dense_min is an fp32 member, printed
    # with the nine digits that give an fp32 back
    want = dict(DEFAULTS, **differ)
    want["dense_min"] = float(np.float32(want["dense_min"]))
    got = dict(got, dense_min=float(np.float32(got["dense_min"])))
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


def test_defaults_and_env_parser_on_every_field(driver):
    exe, _ = driver
    r = subprocess.run([exe, "env"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["env", "ok", "26"], (r.returncode, r.stdout, r.stderr[-2000:])
