"""tools/kernel_res_diff.py on hand-written remark texts: identical builds, one kernel worse, one
kernel missing. The key is the function name: the remarks' line numbers differ throughout."""
import os
import subprocess
import sys

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
sys.path.insert(0, TOOLS)

from kernel_res_diff import diff  # noqa: E402

TAIL = " [-Rpass-analysis=kernel-resource-usage]"


def remarks(line, kernels):
    """Remark text of {name: (sgprs, vgprs, scratch, occupancy)} as hipcc writes it at `line`."""
    out = ["csrc/x.hip:3:9: warning: unused variable 'q' [-Wunused-variable]"]
    for name, (s, v, scratch, occ) in kernels.items():
        pre = f"csrc/x.hip:{line}:1: remark: "
        out += [pre + f"Function Name: {name}" + TAIL, pre + f"    TotalSGPRs: {s}" + TAIL,
                pre + f"    VGPRs: {v}" + TAIL, pre + "    AGPRs: 0" + TAIL,
                pre + f"    ScratchSize [bytes/lane]: {scratch}" + TAIL,
                pre + "    Dynamic Stack: False" + TAIL, pre + f"    Occupancy [waves/SIMD]: {occ}" + TAIL,
                pre + "    SGPRs Spill: 0" + TAIL, pre + "    VGPRs Spill: 0" + TAIL,
                pre + "    LDS Size [bytes/block]: 0" + TAIL]
    return "\n".join(out) + "\n"


OLD = {"k_a": (49, 56, 0, 8), "k_b": (87, 66, 0, 7)}


def test_identical_builds_at_other_lines():
    assert diff(remarks(10, OLD), remarks(99, OLD)) == ([], False)


def test_one_kernel_worse_and_one_better():
    lines, worse = diff(remarks(10, OLD), remarks(99, {"k_a": (49, 72, 0, 7), "k_b": (80, 66, 0, 7)}))
    assert worse
    assert lines == ["worse    k_a: VGPRs 56 -> 72", "worse    k_a: Occupancy [waves/SIMD] 8 -> 7",
                     "better   k_b: TotalSGPRs 87 -> 80"]
    # better alone is no failure; scratch is worse
    assert diff(remarks(10, OLD), remarks(10, {"k_a": (40, 56, 0, 8), "k_b": (87, 66, 0, 8)}))[1] is False
    assert diff(remarks(10, OLD), remarks(10, {"k_a": (49, 56, 16, 8), "k_b": (87, 66, 0, 7)}))[1] is True


def test_one_kernel_missing_and_one_added():
    lines, worse = diff(remarks(10, OLD), remarks(10, {"k_a": OLD["k_a"], "k_c": (10, 10, 0, 8)}))
    assert worse and lines == ["missing  k_b", "added    k_c"]
    assert diff(remarks(10, OLD), remarks(10, dict(OLD, k_c=(10, 10, 0, 8)))) == (["added    k_c"], False)


def test_command_line_exit_status(tmp_path):
    old, same, bad = tmp_path / "old.res", tmp_path / "same.res", tmp_path / "bad.res"
    old.write_text(remarks(10, OLD))
    same.write_text(remarks(20, OLD))
    bad.write_text(remarks(20, {"k_a": OLD["k_a"]}))
    tool = [sys.executable, os.path.join(TOOLS, "kernel_res_diff.py")]
    ok = subprocess.run(tool + [str(old), str(same)], capture_output=True, text=True)
    assert ok.returncode == 0 and ok.stdout.strip() == "no kernel differs"
    ko = subprocess.run(tool + [str(old), str(bad)], capture_output=True, text=True)
    assert ko.returncode == 1 and "missing  k_b" in ko.stdout
