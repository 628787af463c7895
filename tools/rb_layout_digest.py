#!/usr/bin/env python3
"""Digests of the row-block launch layouts of a fixed case table (tests/rb_layout_cases.py), against
tests/golden/mi355x_rb_layout_digests.json: a change that claims to leave layouts alone must
reproduce every digest. GPU.

    python3 tools/rb_layout_digest.py                 # print the cases that differ; rc 1 if any
    python3 tools/rb_layout_digest.py --record --commit <hash of the tree that is recorded>

--diag N adds BSMR_DIAG bits to every case's tuning (1024: the scheduler's decisions on stderr,
which shows the branches each case takes; the layouts do not depend on it).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sddmm-gpu_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="rewrite the golden file")
    ap.add_argument("--commit", default=None, help="with --record: the commit the digests are of")
    ap.add_argument("--out", default=None, help="with --record: write here instead")
    ap.add_argument("--diag", type=int, default=0)
    ap.add_argument("--only", default=None,
                    help="comma-separated case names (with --record: the file keeps its other cases)")
    args = ap.parse_args()
    import torch

    import rb_layout_cases as R
    from bsmr import Plan

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    got = {}
    names = sorted(R.CASES) if args.only is None else args.only.split(",")
    for name in names:
        pat, K, dtype, kw = R.CASES[name]
        kw = dict(kw)
        if args.diag:
            kw["tuning"] = dict(kw.get("tuning", {}), diag=args.diag)
            print(f"== {name}", file=sys.stderr, flush=True)
        M, N, rp, ci = pat()
        plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=R.FREE, **kw)
        w = R.plan_layout_words(plan, K, dtype)
        st = plan.stats()
        got[name] = R.digest(w)
        print(f"{name}: RB {w[0]} NT {w[1]} rowBytes {w[2]} items {w[3]} pieces {w[4]} "
              f"batches {st['rb_batches']} kept tiles {max(st['rb_tiles'])} {got[name][:16]}",
              flush=True)
    if args.record:
        if not args.commit:
            ap.error("--record needs --commit")
        path = args.out or R.GOLDEN
        if args.only is not None:  # the other cases as the golden file has them (same commit and device)
            old = R.load_golden()
            if old["commit"] != args.commit or old["cus"] != cus:
                ap.error("--only: the file was recorded on another commit or device; record all cases")
            got = dict(old["digests"], **got)
        with open(path, "w") as f:
            json.dump({"commit": args.commit, "cus": cus, "digests": got}, f, indent=1,
                      sort_keys=True)
            f.write("\n")
        print(f"recorded {len(got)} digests to {path}")
        return 0
    gold = R.load_golden()
    if gold["cus"] != cus:
        print(f"this device has {cus} CUs, the digests were recorded with {gold['cus']}: "
              "layouts depend on the CU count")
        return 1
    bad = [n for n in got if gold["digests"].get(n) != got[n]]
    for n in bad:
        print(f"DIFFERS: {n}: recorded {gold['digests'].get(n)}, now {got[n]}")
    print(f"{len(got) - len(bad)} of {len(got)} cases match commit {gold['commit']}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
