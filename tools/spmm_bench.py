#!/usr/bin/env python3
"""Times the plan-based SpMM (the SDDMM gradients dA = S(G) B, dB = S(G)^T A) beside the forward
SDDMM and a torch.sparse baseline; one JSON line per case.

    python3 tools/spmm_bench.py [--cases C2,C3] [--steps 50] [--rounds 7] [--sweep]

Per case (C2: nips-like, K = 128, fp32; C3: cop20k-like, K = 256, fp16) and product:
  * graph_us: `steps` launches captured into a HIP graph (as bench.py times the SDDMM), replayed
    for `rounds` rounds in alternation with the other products after a warm-up replay; median
    microseconds per launch;
  * stream_us: the same launches issued on a stream between two events (what the torch baseline
    can be timed as, so the two compare like for like);
  * torch_us: torch.sparse_csr_tensor(...) @ dense on the same tensors, the sparse tensors (S and
    its transpose) built outside the timed region, stream-timed. Where torch lacks the product for
    the dtype the line carries the error text instead of a substitute;
  * floor_us: (8 nnz + 4 K dsts + rowBytes x distinct sources) / 8 TB/s, the byte floor.
--sweep adds the chunk sweep {128, 256, 512, 1024} on C2 side 2 (the skewed side), one plan per
chunk, replayed in alternation.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sddmm-gpu_amd"))

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C2,C3")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from bsmr import F16, F32, Plan, make_data, synth

    assert torch.cuda.is_available(), "spmm_bench needs a GPU"
    dev = torch.device("cuda", 0)
    gs = torch.cuda.Stream(dev)

    def graph_of(fn):
        with torch.cuda.stream(gs):
            fn(gs.cuda_stream)  # warm-up: code objects, lazy builds
        gs.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(gs):
            with torch.cuda.graph(g, stream=gs):
                for _ in range(args.steps):
                    fn(gs.cuda_stream)
            g.replay()
        gs.synchronize()
        return g

    def timed(run):
        with torch.cuda.stream(gs):
            torch.cuda._sleep(200_000)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(gs)
            run()
            e1.record(gs)
        gs.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.steps

    def alternate(runs):
        """{name: median us per launch} of callables replayed in alternation."""
        res = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, r in runs.items():
                res[k].append(timed(r))
        return {k: round(statistics.median(v), 3) for k, v in res.items()}, \
               {k: [round(x, 3) for x in v] for k, v in res.items()}

    def loop(fn):
        def run():
            for _ in range(args.steps):
                fn(gs.cuda_stream)
        return run

    for case in args.cases.split(","):
        if case == "C2":
            (M, N, rp, ci), K, dt, tdt = synth.nips_like(), 128, F32, torch.float32
        elif case == "C3":
            (M, N, rp, ci), K, dt, tdt = synth.cop20k_like(), 256, F16, torch.float16
        else:
            raise SystemExit(f"unknown case {case}")
        nnz = len(ci)
        row_bytes = K * (4 if dt == F32 else 2)
        plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3)
        plan.prepare(K, dt)
        plan.prepare_spmm(K, 3)
        dA = torch.from_numpy(make_data(M * K)).to(dev).to(tdt).reshape(M, K)
        dB = torch.from_numpy(make_data(N * K)).to(dev).to(tdt).reshape(N, K)
        dV = torch.from_numpy(make_data(nnz)).to(dev)
        dP = torch.zeros(nnz, dtype=torch.float32, device=dev)
        dYa = torch.zeros((M, K), dtype=torch.float32, device=dev)
        dYb = torch.zeros((N, K), dtype=torch.float32, device=dev)
        ours = {
            "dA": lambda s: plan.spmm(dV.data_ptr(), dB.data_ptr(), K, dYa.data_ptr(), stream=s, dtype=dt),
            "dB": lambda s: plan.spmm_t(dV.data_ptr(), dA.data_ptr(), K, dYb.data_ptr(), stream=s, dtype=dt),
            "sddmm": lambda s: plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), stream=s, dtype=dt),
        }
        graphs = {k: graph_of(f) for k, f in ours.items()}
        graph_us, graph_all = alternate({k: g.replay for k, g in graphs.items()})
        stream_us, _ = alternate({k: loop(f) for k, f in ours.items()})

        # torch.sparse baseline: sparse tensors built once, outside the timed region
        torch_us, torch_note, check = {}, {}, {}
        crow = torch.from_numpy(rp.astype(np.int64)).to(dev)
        col = torch.from_numpy(ci.astype(np.int64)).to(dev)
        try:
            with torch.cuda.stream(gs):
                S = torch.sparse_csr_tensor(crow, col, dV.to(tdt), size=(M, N))
                St = S.to_sparse_coo().t().coalesce().to_sparse_csr()
            gs.synchronize()
        except Exception as e:  # noqa: BLE001
            S = St = None
            torch_note["build"] = f"{type(e).__name__}: {e}"[:300]
        for name, sp, dense, mine in (("dA", S, dB, dYa), ("dB", St, dA, dYb)):
            if sp is None:
                continue
            try:
                with torch.cuda.stream(gs):
                    ref = sp @ dense  # warm-up, and the values to compare with
                gs.synchronize()
                t, _ = alternate({name: loop(lambda s, sp=sp, dense=dense: sp @ dense)})
                torch_us[name] = t[name]
                d = (ref.float() - mine).abs().max().item()
                check[name] = {"max_abs_diff_vs_torch": d, "max_abs": mine.abs().max().item()}
            except Exception as e:  # noqa: BLE001
                torch_note[name] = f"unsupported by this torch build: {type(e).__name__}: {e}"[:300]

        rows_e = np.repeat(np.arange(M), np.diff(rp.astype(np.int64)))
        floor = {
            "dA": (8 * nnz + 4 * K * M + row_bytes * len(np.unique(ci))) / HBM_BYTES_PER_S * 1e6,
            "dB": (8 * nnz + 4 * K * N + row_bytes * len(np.unique(rows_e))) / HBM_BYTES_PER_S * 1e6,
        }
        line = {"case": case, "M": M, "N": N, "nnz": nnz, "K": K, "dtype": "fp32" if dt == F32 else "fp16",
                "steps": args.steps, "rounds": args.rounds, "graph_us": graph_us, "stream_us": stream_us,
                "torch_us": torch_us, "torch_note": torch_note,
                "floor_us": {k: round(v, 3) for k, v in floor.items()},
                "floor_fraction": {k: round(floor[k] / graph_us[k], 3) for k in floor},
                "spmm_stats": {"rows": plan.spmm_stats(1), "cols": plan.spmm_stats(2)},
                "check": check, "graph_us_rounds": graph_all, "torch": torch.__version__}
        print(json.dumps(line), flush=True)

        if args.sweep and case == "C2":
            plans, runs = [], {}
            for chunk in (128, 256, 512, 1024):
                p = Plan(M, N, rp, ci, alpha=0.3, delta=0.3)
                p.prepare_spmm(K, 2, chunk=chunk)
                plans.append(p)
                g = graph_of(lambda s, p=p: p.spmm_t(dV.data_ptr(), dA.data_ptr(), K, dYb.data_ptr(),
                                                     stream=s, dtype=dt))
                runs[str(chunk)] = g.replay
            med, rounds = alternate(runs)
            print(json.dumps({"case": "C2_chunk_sweep_side2", "K": K, "graph_us": med, "graph_us_rounds": rounds,
                              "stats": {str(p.spmm_stats(2)["chunk"]): p.spmm_stats(2) for p in plans}}),
                  flush=True)


if __name__ == "__main__":
    main()
