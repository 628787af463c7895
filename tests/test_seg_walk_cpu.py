"""CPU: the visiting order of the segment walker of the attention backward (csrc/seg_walk.hpp:
k_attention_bwd_rows and k_attention_bwd_cols walk their segments with it). k_spmm and both phases
of k_attention keep hand-written copies of the same loop; those are held to this order by the GPU
*_float64 tests alone, not by this test.

The walker's control flow is plain C++, so tests/seg_walk_main.cpp instantiates it on the host with
recording functors and runs the 64 lanes of a wave one after the other, for U in {1, 2, 4}, L in
{4, 8, 16, 32, 64} and the counts 0, 1, G - 1, G, G + 1, U G - 1, U G, 63, 64, 65, 127, 128, 129, 256,
257. The properties it holds every case to are listed at the top of that file: they are what the
bit-exact summation order of the backward's *_float64 GPU tests rests on.

The program has its own main and is built with the host compiler under AddressSanitizer and UBSan
and run directly; nothing is loaded into Python. It is compiled on every run, so the build is the
cheap one (-O0, no debug info: a sanitizer report still names the function) and the driver uses no
containers: build and the three runs together are meant to stay under a second.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sddmm-gpu_amd", "csrc")
CASES = 5 * 15  # per unroll depth: L x counts


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("seg_walk_asan") / "seg_walk_main")
    cmd = [cxx, "-std=c++17", "-O0", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "seg_walk_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a linker that cannot find the sanitizer runtimes skips; any other error fails
        if re.search(r"cannot find -l(asan|ubsan)|cannot find .*lib(clang_rt\.)?(asan|ubsan)", r.stderr):
            pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
        raise AssertionError(r.stderr)
    return exe


@pytest.mark.parametrize("unroll", [1, 2, 4])
def test_visiting_order(driver, unroll):
    r = subprocess.run([driver, str(unroll)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip() == f"ok {CASES}", r.stdout[-2000:]
