#!/usr/bin/env python3
"""Compare two files of hipcc's -Rpass-analysis=kernel-resource-usage remarks (build/*.o.res) by
kernel name: prints every kernel whose VGPRs, TotalSGPRs, AGPRs, occupancy, scratch or LDS differ
and every kernel present in one file only. Exit status 1 when a kernel is missing from NEW or worse
in it (more registers, scratch or LDS, lower occupancy), else 0. A kernel that only NEW has is
printed as "added" and does not change the status: where no kernel may be added either, read the
output. Line numbers in the remarks are not part of the key, so code may move.

    python3 tools/kernel_res_diff.py OLD.res NEW.res
"""
import sys

from check_kernel_resources import parse

# field -> +1 when more is worse, -1 when less is worse
FIELDS = {"VGPRs": 1, "TotalSGPRs": 1, "AGPRs": 1, "Occupancy [waves/SIMD]": -1,
          "ScratchSize [bytes/lane]": 1, "LDS Size [bytes/block]": 1}


def diff(old_text, new_text):
    """(lines to print, whether NEW is worse than OLD or lacks one of its kernels)."""
    old, new = parse(old_text), parse(new_text)
    lines, worse = [], False
    for kern in old:
        if kern not in new:
            lines.append(f"missing  {kern}")
            worse = True
            continue
        for field, sign in FIELDS.items():
            a, b = old[kern].get(field, 0), new[kern].get(field, 0)
            if a != b:
                bad = sign * (b - a) > 0
                worse |= bad
                lines.append(f"{'worse ' if bad else 'better'}   {kern}: {field} {a} -> {b}")
    lines += [f"added    {kern}" for kern in new if kern not in old]
    return lines, worse


def main(old_path, new_path):
    with open(old_path, errors="replace") as f, open(new_path, errors="replace") as g:
        lines, worse = diff(f.read(), g.read())
    print("\n".join(lines) if lines else "no kernel differs")
    return 1 if worse else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
