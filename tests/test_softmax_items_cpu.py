"""CPU: the host-only item list of the row softmax (csrc/softmax_schedule.cpp) through
bsmr.softmax_items (bsmr_softmax_items; no plan, no device).

On every pattern of the GPU tests (tests/softmax_cases.py: every row length 0 .. 271, a hub row,
shuffled Zipf rows, empty rows, the smallest legal plans, and `long`, whose rows sit on both sides
of wave_max and block_pass as the library exports them): every non-empty row is in exactly one
item, items ascend, and the list equals, item for item, what numpy derives from the row lengths
and the exported thresholds. A pattern without entries has no item; a malformed rowptr gives
BSMR_ERR_INVALID.

The same source is also built with a stand-alone main (tests/softmax_items_main.cpp) under
AddressSanitizer and UBSan and run on the same patterns; nothing loaded into Python is sanitized.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bsmr
from softmax_cases import PATTERNS, SMALLEST, expected_items, limits, long_lengths, pattern, row_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sddmm-gpu_amd", "csrc")
INVALID = 1  # BSMR_ERR_INVALID
ALL = PATTERNS + SMALLEST


def _fnv(items):
    x = np.asarray(items, np.uint32).ravel().astype(np.uint64)
    i = np.arange(len(x), dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(((x + np.uint64(1)) * (np.uint64(2) * i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)).sum(
            dtype=np.uint64))


def test_limits_are_exported_and_long_straddles_them():
    lim = limits()
    w, b = lim["wave_max"], lim["block_pass"]
    assert 64 < w < b and w % 64 == 0 and b % w == 0
    lens = long_lengths()
    assert {w, w + 1, b, b + 1, 2 * b + 37} <= set(lens) and 0 in lens
    assert list(row_lengths(pattern("long"))) == lens
    assert set(row_lengths(pattern("staircase"))) == set(range(272))


@pytest.mark.parametrize("name", ALL)
def test_items_cover_every_row_once(name):
    pat = pattern(name)
    M, _, rp, _ = pat
    lens = row_lengths(pat)
    w = limits()["wave_max"]
    items = bsmr.softmax_items(M, rp)
    seen = np.zeros(M, np.int64)
    end = 0
    for row, first, count, kind in items.astype(np.int64):
        assert row >= end and first == rp[row]
        if kind <= 64:
            assert kind & (kind - 1) == 0 and 1 <= count <= 64 // kind
            rows = np.arange(row, row + count)
            n = lens[rows]
            assert ((n == 0) | ((n <= kind) & (2 * n > kind))).all()  # one power-of-two class
            assert n[0] > 0 and n[-1] > 0
        else:
            rows = np.array([row])
            assert count == lens[row]
            assert (kind == bsmr.SOFTMAX_WAVE and 64 < count <= w) or (kind == bsmr.SOFTMAX_BLOCK and count > w)
        seen[rows] += 1
        end = rows[-1] + 1
    assert np.array_equal(seen[lens > 0], np.ones((lens > 0).sum(), np.int64)), "a non-empty row not exactly once"
    want = expected_items(pat)
    assert np.array_equal(items, want), (items[:8], want[:8])


def test_kinds_on_the_patterns_that_exist_for_them():
    kinds = {name: set(bsmr.softmax_items(pattern(name)[0], pattern(name)[2])[:, 3].tolist()) for name in PATTERNS}
    assert kinds["staircase"] == {1, 2, 4, 8, 16, 32, 64, bsmr.SOFTMAX_WAVE}
    assert bsmr.SOFTMAX_BLOCK in kinds["hub"] and bsmr.SOFTMAX_BLOCK in kinds["long"] and bsmr.SOFTMAX_WAVE in kinds["long"]
    # a full run of every class: 64 / L consecutive rows of one class in one item
    for L in (1, 2, 4, 8, 16, 32, 64):
        lens = np.full(3 * (64 // L) + 1, L)
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        it = bsmr.softmax_items(len(lens), rp)
        assert it[:, 2].tolist() == [64 // L] * 3 + [1] and (it[:, 3] == L).all(), (L, it)


def test_no_entries_no_items_and_empty_rows_ride_along():
    assert len(bsmr.softmax_items(5, np.zeros(6, np.uint32))) == 0
    assert len(bsmr.softmax_items(0, np.zeros(1, np.uint32))) == 0
    # rows of 3, 0, 0, 4, 0: one run of class 4 over four rows, the trailing empty row left out
    it = bsmr.softmax_items(5, np.array([0, 3, 3, 3, 7, 7], np.uint32))
    assert it.tolist() == [[0, 0, 4, 4]]


def test_malformed_rowptr_is_rejected():
    M, _, rp, _ = pattern("empty")
    for bad in ("first", "swap"):
        rp2 = rp.copy()
        if bad == "first":
            rp2[0] = 1
        else:
            r = int(np.nonzero(np.diff(rp.astype(np.int64)) > 0)[0][0])
            rp2[r], rp2[r + 1] = rp[r + 1], rp[r]
        with pytest.raises(bsmr.BsmrError) as ei:
            bsmr.softmax_items(M, rp2)
        assert ei.value.status == INVALID and "bsmr_softmax_items" in str(ei.value), str(ei.value)
    n = bsmr.C.c_uint64()
    assert bsmr.lib().bsmr_softmax_items(M, None, None, bsmr.C.byref(n)) == INVALID
    assert bsmr.lib().bsmr_softmax_items(M, rp.ctypes.data, None, None) == INVALID


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("softmax_asan")
    exe = str(d / "softmax_items_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "softmax_items_main.cpp"),
           os.path.join(CSRC, "softmax_schedule.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr:
            pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
        raise AssertionError(r.stderr)
    return exe, d


@pytest.mark.parametrize("name", ALL)
def test_sanitized_standalone_build_agrees(driver, name):
    exe, d = driver
    M, _, rp, _ = pattern(name)
    path = str(d / f"{name}.txt")
    with open(path, "w") as f:
        f.write(f"{M}\n" + " ".join(map(str, rp.tolist())) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    items = bsmr.softmax_items(M, rp)
    assert r.stdout.split() == [str(len(items)), f"{_fnv(items):016x}"]
