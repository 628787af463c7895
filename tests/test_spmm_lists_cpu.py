"""CPU: the host-only SpMM gather lists (csrc/spmm_schedule.cpp) through bsmr.spmm_lists
(bsmr_spmm_lists; no plan, no device).

For side 1 (rows) and 2 (columns), chunks 1 / 32 / 512, with and without a launch order, on the
patterns of the GPU tests (Zipf columns, empty rows and columns, one hub row, columns in file
order): the segments hold every stored entry exactly once with its other index as source,
positions ascend inside a destination, no segment exceeds the chunk, every destination has a
segment (an empty one exactly one, of count 0), partial slots are consecutive per split
destination and unused elsewhere, and segments follow the order, then the ascending index. Invalid
inputs give BSMR_ERR_INVALID naming bsmr_spmm_lists.

The same source is also built with a stand-alone main (tests/spmm_lists_main.cpp) under
AddressSanitizer and UBSan and run on the same patterns; nothing is loaded into Python under a
sanitizer.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bsmr
from spmm_cases import PATTERNS, entry_rows, pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sddmm-gpu_amd", "csrc")
INVALID = 1  # BSMR_ERR_INVALID
CHUNKS = [1, 32, 512]


def _order(name, side):
    """A launch order over part of the destinations: a seeded permutation of two thirds."""
    M, N, _, _ = pattern(name)
    D = M if side == 1 else N
    return np.random.default_rng(11).permutation(D)[:2 * D // 3].astype(np.uint32)


def _fnv(*arrays):
    """The driver's digest: sum over the words x_i of (x_i + 1)(2 i + 1) c, modulo 2^64."""
    x = np.concatenate([np.asarray(a, np.uint32).ravel() for a in arrays]).astype(np.uint64)
    i = np.arange(len(x), dtype=np.uint64)
    with np.errstate(over="ignore"):
        terms = (x + np.uint64(1)) * (np.uint64(2) * i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        return int(terms.sum(dtype=np.uint64))


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("name", PATTERNS)
def test_lists_cover_the_pattern(name, side, chunk, ordered):
    M, N, rp, ci = pattern(name)
    nnz = len(ci)
    D = M if side == 1 else N
    order = _order(name, side) if ordered else None
    segs, src, vpos = bsmr.spmm_lists(M, N, rp, ci, side, chunk, order)
    dst, first, count, part = (segs[:, i].astype(np.int64) for i in range(4))
    rows, cols = entry_rows(M, rp), ci.astype(np.int64)
    e_dst, e_src = (rows, cols) if side == 1 else (cols, rows)

    # segments tile [0, nnz) of src / vpos: every stored entry once, with its other index
    assert count.sum() == nnz and (count <= chunk).all()
    slot_dst = np.full(nnz, -1, np.int64)
    for d, f, c in zip(dst, first, count):
        assert (slot_dst[f:f + c] == -1).all()
        slot_dst[f:f + c] = d
    assert (slot_dst >= 0).all()
    assert np.array_equal(np.sort(vpos), np.arange(nnz))
    assert np.array_equal(e_dst[vpos], slot_dst)
    assert np.array_equal(e_src[vpos], src)

    # per destination: at least one segment; an empty one exactly one of count 0; consecutive
    # pieces of its list in launch order, CSR positions ascending across them
    lens = np.bincount(e_dst, minlength=D)
    nseg = np.bincount(dst, minlength=D)
    assert np.array_equal(nseg, np.maximum(1, -(-lens // chunk)))
    assert (count[lens[dst] == 0] == 0).all()
    last_end = {}
    for i, (d, f, c) in enumerate(zip(dst, first, count)):
        if d in last_end:
            assert f == last_end[d] and dst[i - 1] == d  # contiguous in the list and the launch
        last_end[d] = f + c
    starts = np.cumsum(lens) - lens
    for d in np.nonzero(lens)[0]:
        assert (np.diff(vpos[starts[d]:starts[d] + lens[d]].astype(np.int64)) > 0).all()
    assert all(first[i] == starts[dst[i]] for i in range(len(dst)) if i == 0 or dst[i - 1] != dst[i])

    # partial slots: consecutive from 0 over the split destinations in launch order
    split = nseg[dst] > 1
    assert (part[~split] == bsmr.SPMM_DIRECT).all()
    assert np.array_equal(part[split], np.arange(split.sum()))

    # launch order: the order's destinations, then the others ascending
    launched = dst[np.r_[True, dst[1:] != dst[:-1]]]
    head = np.zeros(0, np.int64) if order is None else order.astype(np.int64)
    rest = np.setdiff1d(np.arange(D), head)
    assert np.array_equal(launched, np.r_[head, rest])


def test_invalid_inputs_are_rejected():
    M, N, rp, ci = pattern("empty")

    def bad(**kw):
        a = dict(M=M, N=N, rowptr=rp, colidx=ci, side=1, chunk=32, order=None)
        a.update(kw)
        with pytest.raises(bsmr.BsmrError) as ei:
            bsmr.spmm_lists(**a)
        assert ei.value.status == INVALID and "bsmr_spmm_lists" in str(ei.value), str(ei.value)

    bad(chunk=0)
    bad(side=0)
    bad(side=3)
    bad(order=np.array([0, M], np.uint32))
    bad(side=2, order=np.array([N], np.uint32))
    bad(order=np.array([5, 2, 5], np.uint32))
    rp2 = rp.copy()
    r = int(np.nonzero(np.diff(rp.astype(np.int64)) > 0)[0][0])
    rp2[r], rp2[r + 1] = rp[r + 1], rp[r]
    bad(rowptr=rp2)
    ci2 = ci.copy()
    ci2[len(ci) // 2] = N
    bad(colidx=ci2)
    bad(N=int(ci.max()))


def _sanitized_driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("spmm_asan")
    exe = str(d / "spmm_lists_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "spmm_lists_main.cpp"),
           os.path.join(CSRC, "spmm_schedule.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr:
            pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
        raise AssertionError(r.stderr)
    return exe, d


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _sanitized_driver(tmp_path_factory)


@pytest.mark.parametrize("name", PATTERNS)
def test_sanitized_standalone_build_agrees(driver, name):
    exe, d = driver
    M, N, rp, ci = pattern(name)
    for side in (1, 2):
        for ordered in (False, True):
            order = _order(name, side) if ordered else np.zeros(0, np.uint32)
            path = str(d / f"{name}_{side}_{int(ordered)}.txt")
            with open(path, "w") as f:
                f.write(f"{M} {N} {len(ci)} {len(order)}\n")
                for a in (rp, ci, order):
                    f.write(" ".join(map(str, a.tolist())) + "\n")
            for chunk in CHUNKS:
                r = subprocess.run([exe, path, str(side), str(chunk)], capture_output=True, text=True)
                assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
                segs, src, vpos = bsmr.spmm_lists(M, N, rp, ci, side, chunk, order if ordered else None)
                assert r.stdout.split() == [str(len(segs)), f"{_fnv(segs, src, vpos):016x}"]
