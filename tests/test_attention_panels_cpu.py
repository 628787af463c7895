"""CPU: the host-only panel lists of the MFMA attention forward (csrc/attention_panels.cpp) through
bsmr.attention_panel_lists, in CSR order and in a shuffled order that names only some rows; and the
same source built with a stand-alone main under ASan / UBSan on the same inputs.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import attention_cases as AC
import bsmr
from attention_panels_cases import block_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sddmm-gpu_amd", "csrc")
LIM = bsmr.attention_panels_limits()
DIRECT = 0xFFFFFFFF


def case(name):
    if name == "short_last_panel":  # M = 37: panels of 16, 16 and 5 rows, the second without entries
        lens = np.array([3] * 16 + [0] * 16 + [40, 0, 33, 1, 32])
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        return 37, 64, rp, np.concatenate([np.arange(n) for n in lens]).astype(np.uint32)
    return block_mask() if name == "block_mask" else AC.pattern(name)


CASES = AC.PATTERNS + ["block_mask", "short_last_panel"]


def order_of(name, kind):
    M = case(name)[0]
    return np.arange(M) if kind == "csr" else np.random.default_rng(3).permutation(M)[:M - M // 3]


@pytest.mark.parametrize("kind", ["csr", "shuffled_partial"])
@pytest.mark.parametrize("name", CASES)
def test_lists(name, kind):
    M, N, rp, ci = case(name)
    order = order_of(name, kind)
    rows, cols, masks, items, reds = bsmr.attention_panel_lists(M, N, rp, ci, order)
    assert LIM == dict(step_cols=32, item_steps=LIM["item_steps"]) and cols.shape[1] == 32 and masks.shape[1] == 16
    # the launch order: `order`, then the rows it does not name, ascending
    rest = np.setdiff1d(np.arange(M), order)
    assert np.array_equal(rows, np.concatenate([order, rest]))
    panels = -(-M // 16)
    assert sorted(set(items[:, 0])) == list(range(0, M, 16))
    entries, step, part = [], 0, 0
    for p in range(panels):
        mine = items[items[:, 0] == 16 * p]
        prow = rows[16 * p:16 * p + 16]
        want = [set(ci[rp[r]:rp[r + 1]].tolist()) for r in prow]
        union = sorted(set().union(*want))
        nsteps = -(-len(union) // 32)
        # items tile the panel's steps without gap or overlap, none longer than item_steps
        for it in mine:
            assert it[1] == step and it[2] <= LIM["item_steps"] and (it[2] > 0 or nsteps == 0)
            step += it[2]
        assert mine[:, 2].sum() == nsteps and len(mine) == max(1, -(-nsteps // LIM["item_steps"]))
        s0 = step - nsteps
        flat = cols[s0:step].reshape(-1)
        assert flat[:len(union)].tolist() == union  # ascending, each once
        pad = np.arange(len(union), 32 * nsteps)
        assert (flat[pad] == cols[step - 1, 0]).all() if len(pad) else True  # a column of the same step
        for r in range(16):
            bits = (masks[s0:step, r, None] >> np.arange(32)) & 1
            got = flat[bits.reshape(-1) == 1]
            assert not bits.reshape(-1)[pad].any()
            assert got.tolist() == (sorted(want[r]) if r < len(prow) else [])
            entries.append(len(got))
        # split panels and the reduce list agree
        if len(mine) > 1:
            red = reds[reds[:, 0] == 16 * p]
            assert red.tolist() == [[16 * p, part, len(mine), 0]]
            assert mine[:, 3].tolist() == list(range(part, part + len(mine)))
            part += len(mine)
        else:
            assert mine[0, 3] == DIRECT and not (reds[:, 0] == 16 * p).any()
    assert step == len(cols) and sum(entries) == len(ci) and len(reds) == len(set(reds[:, 0]))
    if name == "block_mask" and kind == "csr":  # (a shuffled order mixes block rows in a panel)
        assert 1000 * len(ci) // (16 * 32 * len(cols)) == 1000
    if name == "short_last_panel" and kind == "csr":
        assert items.tolist() == [[0, 0, 1, DIRECT], [16, 1, 0, DIRECT], [32, 1, 2, DIRECT]]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("panels_asan")
    exe = str(d / "attention_panels_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "attention_panels_main.cpp"),
           os.path.join(CSRC, "attention_panels.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr:
            pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
        raise AssertionError(r.stderr)
    return exe, d


@pytest.mark.parametrize("name", CASES)
def test_sanitized_standalone_build_agrees(driver, name):
    exe, d = driver
    M, N, rp, ci = case(name)
    order = order_of(name, "shuffled_partial")
    path = str(d / f"{name}.txt")
    with open(path, "w") as f:
        f.write(f"{M} {N} {len(order)}\n" + "\n".join(" ".join(map(str, np.asarray(x).tolist())) for x in (rp, ci, order)))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    rows, cols, masks, items, reds = bsmr.attention_panel_lists(M, N, rp, ci, order)
    steps = np.concatenate([cols, masks], axis=1)
    want = [" ".join([k] + [str(v) for v in x.reshape(-1).tolist()]) for k, x in
            (("rows", rows), ("steps", steps), ("items", items), ("reds", reds))]
    assert r.stdout.splitlines() == want
