#!/usr/bin/env python3
"""Build gate: parse hipcc's -Rpass-analysis=kernel-resource-usage remarks and fail when an SDDMM
kernel (k_sddmm*, k_sim_filter, k_spmm*, k_softmax*, k_attention*) spills VGPRs/SGPRs or uses scratch. Usage: check_kernel_resources.py <remarks>"""
import os
import re
import sys


GATED = ("k_sddmm", "k_sim_filter", "k_spmm", "k_softmax", "k_attention")


def gated(kern):
    return any(g in kern for g in GATED)


def parse(text):
    """{function name: {remark field: value}} of the remarks in `text`, integer fields only (e.g.
    "VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]", "ScratchSize [bytes/lane]"), in file order."""
    out, kern = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            kern = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([^:]+): (\d+) \[-Rpass", line)
        if m and kern is not None:
            kern[m.group(1)] = int(m.group(2))
    return out


def parse_file(path):
    with open(path, errors="replace") as f:
        return parse(f.read())


def main(path):
    kernels = {k: v for k, v in parse_file(path).items() if gated(k)}
    allow = os.environ.get("RES_CHECK_ALLOW")  # experiments only: a regex of kernels
    bad = [f"{kern}: {field} = {res[field]}" for kern, res in kernels.items()
           if not (allow and re.search(allow, kern))
           for field in ("VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]") if res.get(field, 0) > 0]
    if bad:
        sys.stderr.write("kernel resource check failed (spills/scratch):\n  " + "\n  ".join(bad) + "\n")
        return 1
    if not kernels:
        sys.stderr.write(f"kernel resource check: no k_sddmm / k_sim_filter / k_spmm / k_softmax / k_attention kernels in {path}\n")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
