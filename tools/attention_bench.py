#!/usr/bin/env python3
"""Times the row softmax over the plan's pattern (forward, backward), the whole sparse attention
forward + backward, and the attention forward alone as the composed chain and as the one fused
launch, beside the byte floors and the same softmax written with torch ops; one JSON line per case.

    python3 tools/attention_bench.py [--cases C2,C3] [--steps 50] [--rounds 7] [--d 64]

Per case (the C2 nips-like and C3 cop20k-like stand-in patterns, fp32, D = Dv = --d):
  * graph_us: `steps` calls captured into a HIP graph (as bench.py times the SDDMM), replayed for
    `rounds` rounds in alternation after a warm-up replay; median microseconds per call.
      softmax_fwd / softmax_bwd: one Plan.softmax / Plan.softmax_backward;
      attention: the eight launches of attention forward + backward on preallocated buffers (sddmm,
      softmax, spmm; then sddmm and spmm_t for dW and dV, softmax_backward, spmm and spmm_t for dQ
      and dK): the hand composition that tests/test_gpu_attention_autograd.py shows bitwise equal
      to bsmr.autograd.attention, without the autograd allocations a capture would not time fairly;
      composed_fwd: its first three launches (sddmm, softmax, spmm) on the same tensors;
      fused_fwd: one Plan.attention on the same tensors (O and LSE written);
  * stream_us: the same calls issued on a stream between two events (how the torch chain is timed,
    so the two compare like for like);
  * torch_us: the softmax as a chain of torch ops on the same tensors, stream-timed: forward
    scatter_reduce(amax), gather, exp, index_add, gather, divide; backward index_add of W G, gather,
    two products. Its result is compared with ours (max_abs_diff);
  * floor_us: 8 nnz + 4 (M + 1) bytes forward (P read, W written, rowptr) and 16 nnz + 4 (M + 1)
    backward (W and G read, dP written, and 4 nnz allowed for the second read of rows longer than
    one pass), over 8 TB/s; fused_fwd: Q and O, one read of every K and V row that some entry
    references, colidx and LSE; floor_fraction = floor / graph;
  * fused_over_composed: graph_us of fused_fwd / composed_fwd, and the largest |O_fused - O_composed|;
  * the backward alone, three ways on the same tensors (graph_us, stream_us, floor_us; launches: the
    library calls of each and the kernels of the fused call):
      composed_bwd: the five launches of attention's backward after a forward that kept P and W
      (sddmm and spmm_t for dW and dV, softmax_backward, spmm and spmm_t for dQ and dK);
      recompute_bwd: sddmm and softmax again, then those five (attention_fused's default backward);
      fused_bwd: one Plan.attention_backward from O and LSE (delta, rows, columns and the reduces of
      split destinations: at most five launches, no nnz-sized tensor);
    floors: every dense operand and gradient once (Q, K, V, GO and dQ, dK, dV; the fused one also O)
    and the nnz-sized traffic each path cannot avoid: 28 nnz bytes composed (dW written and read, W
    read twice, dP written and read twice), 40 nnz recompute (P written and read, W written), 8 nnz
    fused (the column index of every entry on the row side, its row on the column side);
    backward_peak_bytes: torch's peak over forward + backward through bsmr.autograd (attention,
    attention_fused, attention_fused(backward="fused")) above what was allocated before;
    attention_backward_stats carries the plan-owned scratch of the fused backward.
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
    ap.add_argument("--d", type=int, default=64)
    args = ap.parse_args()
    import numpy as np
    import torch

    from bsmr import Plan, make_data, synth

    assert torch.cuda.is_available(), "attention_bench needs a GPU"
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
        res = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, r in runs.items():
                res[k].append(timed(r))
        return {k: round(statistics.median(v), 3) for k, v in res.items()}

    def loop(fn):
        def run():
            for _ in range(args.steps):
                fn(gs.cuda_stream)
        return run

    D = args.d
    scale = D ** -0.5
    for case in args.cases.split(","):
        if case == "C2":
            M, N, rp, ci = synth.nips_like()
        elif case == "C3":
            M, N, rp, ci = synth.cop20k_like()
        else:
            raise SystemExit(f"unknown case {case}")
        nnz = len(ci)
        plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3)
        plan.prepare(D)
        plan.prepare_spmm(D, 3)
        plan.prepare_softmax()
        plan.prepare_attention(D, D)
        plan.prepare_attention_backward(D, D)

        def data(n, shape=None):
            t = torch.from_numpy(make_data(n)).to(dev) - 1.0  # uniform [-1, 1)
            return t.reshape(shape) if shape else t

        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        Q, K, V, dO = data(M * D, (M, D)), data(N * D, (N, D)), data(N * D, (N, D)), data(M * D, (M, D))
        P, G = data(nnz) * 8.0, data(nnz)
        W, gP = z(nnz), z(nnz)
        aP, aW, aO, agW, agV, agP, agQ, agK = z(nnz), z(nnz), z(M, D), z(nnz), z(N, D), z(nnz), z(M, D), z(N, D)
        p = lambda t: t.data_ptr()  # noqa: E731

        def attention(s):
            plan.sddmm(p(Q), p(K), D, p(aP), stream=s)
            plan.softmax(p(aP), p(aW), scale, stream=s)
            plan.spmm(p(aW), p(V), D, p(aO), stream=s)
            plan.sddmm(p(dO), p(V), D, p(agW), stream=s)
            plan.spmm_t(p(aW), p(dO), D, p(agV), stream=s)
            plan.softmax_backward(p(aW), p(agW), p(agP), scale, stream=s)
            plan.spmm(p(agP), p(K), D, p(agQ), stream=s)
            plan.spmm_t(p(agP), p(Q), D, p(agK), stream=s)

        fO, fL = z(M, D), z(M)

        def composed_fwd(s):
            plan.sddmm(p(Q), p(K), D, p(aP), stream=s)
            plan.softmax(p(aP), p(aW), scale, stream=s)
            plan.spmm(p(aW), p(V), D, p(aO), stream=s)

        def fused_fwd(s):
            plan.attention(p(Q), p(K), p(V), D, D, p(fO), p(fL), scale, stream=s)

        bgQ, bgK, bgV = z(M, D), z(N, D), z(N, D)

        def composed_bwd(s):
            plan.sddmm(p(dO), p(V), D, p(agW), stream=s)
            plan.spmm_t(p(aW), p(dO), D, p(agV), stream=s)
            plan.softmax_backward(p(aW), p(agW), p(agP), scale, stream=s)
            plan.spmm(p(agP), p(K), D, p(agQ), stream=s)
            plan.spmm_t(p(agP), p(Q), D, p(agK), stream=s)

        def recompute_bwd(s):
            plan.sddmm(p(Q), p(K), D, p(aP), stream=s)
            plan.softmax(p(aP), p(aW), scale, stream=s)
            composed_bwd(s)

        def fused_bwd(s):
            plan.attention_backward(p(Q), p(K), p(V), p(fO), p(dO), p(fL), D, D, p(bgQ), p(bgK), p(bgV), scale, stream=s)

        ours = {
            "softmax_fwd": lambda s: plan.softmax(p(P), p(W), scale, stream=s),
            "softmax_bwd": lambda s: plan.softmax_backward(p(W), p(G), p(gP), scale, stream=s),
            "attention": attention,
            "composed_fwd": composed_fwd,
            "fused_fwd": fused_fwd,
            "composed_bwd": composed_bwd,
            "recompute_bwd": recompute_bwd,
            "fused_bwd": fused_bwd,
        }
        graphs = {k: graph_of(f) for k, f in ours.items()}
        graph_us = alternate({k: g.replay for k, g in graphs.items()})
        stream_us = alternate({k: loop(f) for k, f in ours.items()})

        rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp.astype(np.int64)))).to(dev)

        def torch_fwd(_s=None):
            m = torch.full((M,), float("-inf"), device=dev).scatter_reduce(0, rows, P, "amax")
            t = torch.exp((P - m[rows]) * scale)
            return t / torch.zeros(M, device=dev).index_add_(0, rows, t)[rows]

        def torch_bwd(_s=None):
            r = torch.zeros(M, device=dev).index_add_(0, rows, W * G)
            return scale * W * (G - r[rows])

        with torch.cuda.stream(gs):
            tW, tgP = torch_fwd(), torch_bwd()
        gs.synchronize()
        torch_us = alternate({"softmax_fwd": loop(torch_fwd), "softmax_bwd": loop(torch_bwd)})
        check = {"softmax_fwd_max_abs_diff_vs_torch": (tW - W).abs().max().item(),
                 "softmax_bwd_max_abs_diff_vs_torch": (tgP - gP).abs().max().item()}

        used = len(np.unique(ci))  # K and V rows that some entry references
        floor = {"softmax_fwd": (8 * nnz + 4 * (M + 1)) / HBM_BYTES_PER_S * 1e6,
                 "softmax_bwd": (16 * nnz + 4 * (M + 1)) / HBM_BYTES_PER_S * 1e6,
                 "fused_fwd": (4 * D * (2 * M + 2 * used) + 4 * nnz + 4 * M) / HBM_BYTES_PER_S * 1e6}
        with torch.cuda.stream(gs):
            composed_fwd(gs.cuda_stream)
            fused_fwd(gs.cuda_stream)
        gs.synchronize()
        check["fused_vs_composed_max_abs_diff"] = (fO - aO).abs().max().item()
        with torch.cuda.stream(gs):
            composed_bwd(gs.cuda_stream)
            fused_bwd(gs.cuda_stream)
        gs.synchronize()
        for name, a, b in (("dQ", bgQ, agQ), ("dK", bgK, agK), ("dV", bgV, agV)):
            check[f"fused_vs_composed_bwd_{name}_max_abs_diff"] = (a - b).abs().max().item()
        bst = plan.attention_backward_stats()
        dense = 4 * D * (M + 2 * used + M) + 4 * D * (M + 2 * N)  # Q, K, V, GO read; dQ, dK, dV written
        floor["composed_bwd"] = (dense + 28 * nnz) / HBM_BYTES_PER_S * 1e6
        floor["recompute_bwd"] = (dense + 40 * nnz) / HBM_BYTES_PER_S * 1e6
        floor["fused_bwd"] = (dense + 4 * D * M + 8 * nnz + 12 * M) / HBM_BYTES_PER_S * 1e6
        # library calls per backward, and the kernels of the one fused call (delta, rows, columns, two reduces)
        launches = {"composed_bwd_calls": 5, "recompute_bwd_calls": 7, "fused_bwd_calls": 1,
                    "fused_bwd_kernels": 3 + (bst["row_split"] > 0) + (bst["col_split"] > 0)}

        from bsmr import autograd

        def peak(fn):
            ts = [t.clone().requires_grad_() for t in (Q, K, V)]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            fn(*ts).backward(dO)
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - before

        peaks = {}
        for name, fn in (("attention", lambda q, k, v: autograd.attention(plan, q, k, v)),
                         ("attention_fused_recompute", lambda q, k, v: autograd.attention_fused(plan, q, k, v)),
                         ("attention_fused_fused", lambda q, k, v: autograd.attention_fused(plan, q, k, v, backward="fused"))):
            peak(fn)  # warm the allocator
            peaks[name] = peak(fn)
        line = {"case": case, "M": M, "N": N, "nnz": nnz, "D": D, "scale": scale, "steps": args.steps,
                "rounds": args.rounds, "graph_us": graph_us, "stream_us": stream_us, "torch_us": torch_us,
                "floor_us": {k: round(v, 3) for k, v in floor.items()},
                "floor_fraction": {k: round(floor[k] / graph_us[k], 3) for k in floor},
                "torch_over_ours_stream": {k: round(torch_us[k] / stream_us[k], 2) for k in torch_us},
                "fused_over_composed": round(graph_us["fused_fwd"] / graph_us["composed_fwd"], 3),
                "softmax_stats": plan.softmax_stats(), "attention_stats": plan.attention_stats(),
                "launches": launches, "backward_peak_bytes": peaks, "nnz_bytes": 4 * nnz, "attention_backward_stats": bst,
                "fused_bwd_over_composed_bwd": round(graph_us["fused_bwd"] / graph_us["composed_bwd"], 3),
                "fused_bwd_over_recompute_bwd": round(graph_us["fused_bwd"] / graph_us["recompute_bwd"], 3), "check": check, "torch": torch.__version__}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
