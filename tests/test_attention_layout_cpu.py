"""CPU: the host-only layout rules of the strided attention operands (csrc/attention_layout.cpp)
through bsmr.attention_layout_check (bsmr_attention_layout_check; no plan, no device).

One table of accepted and refused layouts (CASES), each against the rule it exists for: dense
(B, H, M, W) and (B, M, H, W), padded rows, input strides of 0, extent-1 dimensions with arbitrary
strides; a null operand, a null and a misaligned pointer, strides off the 16-byte rule, row < W, an
output with a stride of 0, an output whose head range overlaps the next row, 64-bit overflow of the
last offset, extents of 0 and of limit + 1.

The same source is also built with a stand-alone main (tests/attention_layout_main.cpp) under
AddressSanitizer and UBSan and run on the same table; nothing loaded into Python is sanitized.
"""
import os
import shutil
import subprocess

import pytest

import bsmr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sddmm-gpu_amd", "csrc")
INVALID = 1  # BSMR_ERR_INVALID
P = 1 << 20  # a 16-byte aligned address; nothing is dereferenced
LIM = bsmr.attention_heads_limits()
MAXB, MAXH = LIM["max_batches"], LIM["max_heads"]
B, H, M, W = 2, 3, 10, 32

# name: (ptr | None for the null operand, batch, head, row, batches, heads, rows, width, elem_bytes,
#        is_output, accepted, a word of the message when refused)
CASES = {
    # ---- accepted
    "dense_bhmd_in": (P, H * M * W, M * W, W, B, H, M, W, 4, 0, True, ""),
    "dense_bhmd_out": (P, H * M * W, M * W, W, B, H, M, W, 4, 1, True, ""),
    "dense_bmhd_in": (P, M * H * W, W, H * W, B, H, M, W, 2, 0, True, ""),
    "dense_bmhd_out": (P, M * H * W, W, H * W, B, H, M, W, 4, 1, True, ""),
    "padded_row_out": (P, H * M * (W + 8), M * (W + 8), W + 8, B, H, M, W, 4, 1, True, ""),
    "padded_bmhd_out": (P, M * (H * W + 16) + 64, W, H * W + 16, B, H, M, W, 4, 1, True, ""),
    "padded_half_in": (P, H * M * (W + 8), M * (W + 8), W + 8, B, H, M, W, 2, 0, True, ""),
    "head_stride_0_in": (P, M * W, 0, W, B, H, M, W, 4, 0, True, ""),
    "batch_and_head_stride_0_in": (P, 0, 0, W, B, H, M, W, 2, 0, True, ""),
    "extent_1_arbitrary_strides_in": (P, 7, 3, 5, 1, 1, 1, W, 4, 0, True, ""),
    "extent_1_arbitrary_strides_out": (P, 1, 3, W, 1, 1, M, W, 4, 1, True, ""),
    "extent_1_batch_out": (P, 5, M * W, W, 1, H, M, W, 4, 1, True, ""),
    "one_row_any_row_stride_out": (P, H * W, W, 1, B, H, 1, W, 4, 1, True, ""),
    "limits_themselves": (P, 0, 0, W, MAXB, MAXH, M, W, 4, 0, True, ""),
    "row_stride_just_under_2_32_bytes": (P, 0, 0, (1 << 30) - 4, 1, 1, 2, W, 4, 0, True, ""),
    "far_head_in": (P, 0, (1 << 30) + 64, W, 1, 2, M, W, 4, 0, True, ""),
    # ---- refused
    "null_operand": (None, 0, 0, W, 1, 1, M, W, 4, 0, False, "null operand"),
    "null_pointer": (0, H * M * W, M * W, W, B, H, M, W, 4, 0, False, "null device pointer"),
    "misaligned_pointer": (P + 8, H * M * W, M * W, W, B, H, M, W, 4, 0, False, "aligned"),
    "row_stride_not_16_bytes": (P, H * M * (W + 2), M * (W + 2), W + 2, B, H, M, W, 4, 0, False, "row stride"),
    "head_stride_not_16_bytes": (P, 4096, M * W + 4, W, B, H, M, W, 2, 0, False, "head stride"),
    "batch_stride_not_16_bytes": (P, H * M * W + 1, M * W, W, B, H, M, W, 4, 0, False, "batch stride"),
    "row_below_width": (P, H * M * W, M * W, W - 4, B, H, M, W, 4, 0, False, "below the row width"),
    "row_stride_0_in": (P, H * M * W, M * W, 0, B, H, M, W, 4, 0, False, "below the row width"),
    "row_stride_2_32_bytes": (P, 0, 0, 1 << 30, 1, 1, 2, W, 4, 0, False, "2^32"),
    "head_stride_0_out": (P, M * W, 0, W, B, H, M, W, 4, 1, False, "overlap"),
    "batch_stride_0_out": (P, 0, M * W, W, B, H, M, W, 4, 1, False, "overlap"),
    # bmhd whose row stride holds only two of the three heads: head 2 of a row is head 0 of the next
    "head_range_overlaps_next_row_out": (P, M * H * W, W, 2 * W, B, H, M, W, 4, 1, False, "overlap"),
    "batch_inside_heads_out": (P, M * W, M * W, W, B, H, M, W, 4, 1, False, "overlap"),
    "head_below_width_out": (P, M * H * W, W - 4, H * W, B, H, M, W, 4, 1, False, "overlap"),
    "overflow_batch_times_extent": (P, 1 << 62, M * W, W, 8, H, M, W, 4, 0, False, "64 bits"),
    "overflow_stride_bytes": (P, 1 << 62, M * W, W, 2, H, M, W, 4, 0, False, "64 bits"),
    "overflow_last_byte": (P, ((1 << 62) - (1 << 10)), 0, W, 2, H, M, W, 4, 0, False, "64 bits"),
    "overflow_sum_of_spans": (P, (1 << 63) // 4 - 64, (1 << 63) // 4 - 64, W, 3, 3, M, W, 2, 0, False, "64 bits"),
    "overflow_pointer_plus_offset": ((1 << 64) - 4096, 0, 0, W, 1, 1, 1 << 20, W, 4, 0, False, "64 bits"),
    "batches_0": (P, H * M * W, M * W, W, 0, H, M, W, 4, 0, False, "batches"),
    "heads_0": (P, H * M * W, M * W, W, B, 0, M, W, 4, 0, False, "heads"),
    "batches_limit_plus_1": (P, 0, 0, W, MAXB + 1, H, M, W, 4, 0, False, "batches"),
    "heads_limit_plus_1": (P, 0, 0, W, B, MAXH + 1, M, W, 4, 0, False, "heads"),
    "rows_0": (P, H * M * W, M * W, W, B, H, 0, W, 4, 0, False, "positive"),
    "width_0": (P, H * M * W, M * W, W, B, H, M, 0, 4, 0, False, "positive"),
}


def _call(case):
    ptr, batch, head, row, nb, nh, rows, width, esz, out, _, _ = case
    op = None if ptr is None else (ptr, batch, head, row)
    return bsmr.attention_layout_check(op, nb, nh, rows, width, esz, bool(out))


def test_limits_are_exported():
    assert LIM == dict(max_batches=65535, max_heads=65535)
    header = open(os.path.join(ROOT, "include", "bsmr.h")).read()
    assert "#define BSMR_ATTENTION_MAX_BATCHES 65535u" in header and "#define BSMR_ATTENTION_MAX_HEADS   65535u" in header
    assert bsmr.C.sizeof(bsmr.AttentionOperand) == 32
    # the existing limit dicts are left alone
    assert set(bsmr.attention_limits()) == {"chunk", "max_row_bytes"}
    assert set(bsmr.attention_backward_limits()) == {"row_chunk", "col_chunk", "max_row_bytes"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_layout_rules(name):
    case = CASES[name]
    msg = _call(case)
    if case[10]:
        assert msg is None, msg
    else:
        assert msg is not None, "accepted"
        assert msg.startswith("bsmr_attention_layout_check: operand: ") and case[11] in msg, msg
        # the status itself
        ptr, batch, head, row, nb, nh, rows, width, esz, out, _, _ = case
        op = None if ptr is None else bsmr.C.byref(bsmr.AttentionOperand(ptr, batch, head, row))
        assert bsmr.lib().bsmr_attention_layout_check(op, nb, nh, rows, width, esz, out) == INVALID


def test_an_input_rule_set_is_a_subset_of_the_output_rule_set():
    """Whatever is accepted as an output is accepted as an input."""
    for name, case in CASES.items():
        if case[9] and case[10]:
            assert _call(case[:9] + (0,) + case[10:]) is None, name


def test_tensor_views_map_to_operands():
    torch = pytest.importorskip("torch")
    x = torch.empty(B, M, H * W)
    v = x.view(B, M, H, W).transpose(1, 2)
    o = bsmr.AttentionOperand.of(v)
    assert (o.ptr, o.batch, o.head, o.row) == (x.data_ptr(), M * H * W, W, H * W)
    k = torch.empty(M, W).expand(H, M, W)
    o = bsmr.AttentionOperand.of(k)
    assert (o.batch, o.head, o.row) == (0, 0, W)
    with pytest.raises(ValueError):
        bsmr.AttentionOperand.of(x.view(B, M, H, W).permute(0, 2, 3, 1))
    with pytest.raises(ValueError):
        bsmr.AttentionOperand.of(torch.empty(M, W))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("layout_asan")
    exe = str(d / "attention_layout_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "attention_layout_main.cpp"), os.path.join(CSRC, "attention_layout.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr:
            pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
        raise AssertionError(r.stderr)
    return exe, d


def test_sanitized_standalone_build_agrees(driver):
    exe, d = driver
    names = sorted(CASES)
    path = str(d / "table.txt")
    with open(path, "w") as f:
        for n in names:
            c = CASES[n]
            f.write(" ".join(["null" if c[0] is None else str(c[0])] + [str(x) for x in c[1:10]]) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(names)
    for n, line in zip(names, lines):
        msg = _call(CASES[n])
        want = "0" if msg is None else "1 " + msg[len("bsmr_attention_layout_check: operand: "):]
        assert line == want, (n, line, want)
        assert (line == "0") == CASES[n][10], n
