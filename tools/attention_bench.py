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

    python3 tools/attention_bench.py --heads H --batches B [--dtype f32|f16] [--layout bmhd|bhmd]
                                     [--baseline-only] [--package DIR]

With --heads / --batches (Z = B H slices of the case's pattern) the tool times,
by the same protocol (graphs of `steps`, median of `rounds` alternating replays), forward and fused
backward:
  * heads_fwd / heads_bwd: one Plan.attention_heads / Plan.attention_backward_heads call on views of
    (B, M, H D) projections (--layout bmhd: head stride D, row stride H D) or on dense (B, H, M, D);
  * seq_fwd / seq_bwd: Z sequential single-slice Plan.attention / Plan.attention_backward calls on
    contiguous per-slice copies (the copies are made before, not timed);
  * heads_over_seq, floor_us (every slice's dense operands and outputs once, the K and V rows some
    entry references, LSE and delta, and the index arrays once: 4 nnz forward, 8 nnz backward) and
    the plan-owned scratch per slice in bytes.
--order-probe adds four split forms of the backward that tell the launch order from the grid (each
is the row side, GQ alone, and the column side, GK and GV alone; delta runs in both):
  seq_split_slice_major   per slice the row-side call, then the column-side call (a slice's operands
                          are reused between its kernels, as in seq_bwd);
  seq_split_kernel_major  the row-side calls of all Z slices, then the column-side calls of all Z;
  heads_split             one row-side heads call, then one column-side heads call;
  heads_rows / heads_cols those two calls alone, beside seq_rows / seq_cols (Z single-slice calls each).
--baseline-only times the sequential form alone and needs no heads entry point; with --package DIR
(a directory holding a bsmr package with its built library, e.g. a checkout of another commit) that
form can be taken from another build in the same session, for A/B runs.
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
    ap.add_argument("--heads", type=int, default=0)
    ap.add_argument("--batches", type=int, default=0)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16"])
    ap.add_argument("--layout", default="bmhd", choices=["bmhd", "bhmd"])
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--order-probe", action="store_true")
    ap.add_argument("--package", default=None)
    args = ap.parse_args()
    if args.package:
        sys.path.insert(0, os.path.abspath(args.package))
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
    if args.heads or args.batches:
        heads_bench(args, torch, np, dev, graph_of, alternate)
        return
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


def heads_bench(args, torch, np, dev, graph_of, alternate):
    """The --heads / --batches mode (module docstring)."""
    import bsmr
    from bsmr import F16, F32, Plan, make_data, synth

    B, H, D = max(args.batches, 1), max(args.heads, 1), args.d
    Z = B * H
    scale = D ** -0.5
    tdt, dtype, esz = (torch.float32, F32, 4) if args.dtype == "f32" else (torch.float16, F16, 2)
    p = lambda t: t.data_ptr()  # noqa: E731
    for case in args.cases.split(","):
        if case not in ("C2", "C3"):
            raise SystemExit(f"unknown case {case}")
        M, N, rp, ci = synth.nips_like() if case == "C2" else synth.cop20k_like()
        nnz = len(ci)
        plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3)
        plan.prepare_attention(D, D)
        plan.prepare_attention_backward(D, D)

        def data(rows):
            t = (torch.from_numpy(make_data(B * rows * H * D)).to(dev) - 1.0).reshape(B, rows, H, D)
            if args.layout == "bhmd":
                t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
            return t.to(tdt)

        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        like = lambda t: torch.zeros_like(t, dtype=torch.float32)  # noqa: E731
        # (B, H, rows, D) views of the chosen layout
        bQ, bK, bV, bdO = data(M), data(N), data(N), data(M).float()
        Q, K, V, dO = (t.permute(0, 2, 1, 3) for t in (bQ, bK, bV, bdO))
        O, gQ, gK, gV = (like(t).permute(0, 2, 1, 3) for t in (bQ, bQ, bK, bV))
        L = z(B, H, M)
        slices = [(b, h) for b in range(B) for h in range(H)]
        sQ, sK, sV, sdO = ([t[b, h].contiguous() for b, h in slices] for t in (Q, K, V, dO))
        sO, sgQ, sgK, sgV = ([z(r, D) for _ in slices] for r in (M, M, N, N))
        sL = [z(M) for _ in slices]

        def seq_fwd(s):
            for i in range(Z):
                plan.attention(p(sQ[i]), p(sK[i]), p(sV[i]), D, D, p(sO[i]), p(sL[i]), scale, stream=s, dtype=dtype)

        def seq_bwd(s):
            for i in range(Z):
                plan.attention_backward(p(sQ[i]), p(sK[i]), p(sV[i]), p(sO[i]), p(sdO[i]), p(sL[i]), D, D, p(sgQ[i]),
                                        p(sgK[i]), p(sgV[i]), scale, stream=s, dtype=dtype)

        ours = {"seq_fwd": seq_fwd, "seq_bwd": seq_bwd}
        if not args.baseline_only:
            plan.prepare_attention_heads(D, D, Z)
            plan.prepare_attention_backward_heads(D, D, Z)
            ours["heads_fwd"] = lambda s: plan.attention_heads(B, H, Q, K, V, D, D, O, p(L), scale, stream=s, dtype=dtype)
            ours["heads_bwd"] = lambda s: plan.attention_backward_heads(B, H, Q, K, V, O, dO, p(L), D, D, gQ, gK, gV, scale,
                                                                        stream=s, dtype=dtype)
        if args.order_probe and not args.baseline_only:
            def seq_side(i, s, rows):
                plan.attention_backward(p(sQ[i]), p(sK[i]), p(sV[i]), p(sO[i]), p(sdO[i]), p(sL[i]), D, D,
                                        p(sgQ[i]) if rows else 0, 0 if rows else p(sgK[i]), 0 if rows else p(sgV[i]), scale,
                                        stream=s, dtype=dtype)

            def heads_side(s, rows):
                plan.attention_backward_heads(B, H, Q, K, V, O, dO, p(L), D, D, gQ if rows else None, None if rows else gK,
                                              None if rows else gV, scale, stream=s, dtype=dtype)

            def slice_major(s):
                for i in range(Z):
                    seq_side(i, s, True)
                    seq_side(i, s, False)

            def kernel_major(s, sides=(True, False)):
                for rows in sides:
                    for i in range(Z):
                        seq_side(i, s, rows)

            ours.update({"seq_split_slice_major_bwd": slice_major, "seq_split_kernel_major_bwd": kernel_major,
                         "heads_split_bwd": lambda s: (heads_side(s, True), heads_side(s, False)),
                         "seq_rows_bwd": lambda s: kernel_major(s, (True,)), "seq_cols_bwd": lambda s: kernel_major(s, (False,)),
                         "heads_rows_bwd": lambda s: heads_side(s, True), "heads_cols_bwd": lambda s: heads_side(s, False)})
        # forward first: the backward reads O and LSE
        graphs = {k: graph_of(ours[k]) for k in sorted(ours, key=lambda k: k.endswith("bwd"))}
        graph_us = alternate({k: g.replay for k, g in graphs.items()})
        used = len(np.unique(ci))
        inputs = esz * D * (M + 2 * used)
        floor = {"fwd": (Z * (inputs + 4 * D * M + 4 * M) + 4 * nnz) / HBM_BYTES_PER_S * 1e6,
                 "bwd": (Z * (inputs + 8 * D * M + 4 * D * (M + 2 * N) + 12 * M) + 8 * nnz) / HBM_BYTES_PER_S * 1e6}
        line = {"case": case, "mode": "heads", "M": M, "N": N, "nnz": nnz, "D": D, "dtype": args.dtype, "batches": B,
                "heads": H, "slices": Z, "layout": args.layout, "steps": args.steps, "rounds": args.rounds,
                "package": os.path.dirname(os.path.abspath(bsmr.__file__)), "graph_us": graph_us,
                "floor_us": {k: round(v, 3) for k, v in floor.items()}}
        if not args.baseline_only:
            same = all(torch.equal(O[b, h], sO[i]) and torch.equal(gK[b, h], sgK[i]) for i, (b, h) in enumerate(slices))
            ast, bst = plan.attention_stats(), plan.attention_backward_stats()
            line.update({"heads_over_seq": {d: round(graph_us[f"heads_{d}"] / graph_us[f"seq_{d}"], 3) for d in ("fwd", "bwd")},
                         "floor_fraction": {d: round(floor[d] / graph_us[f"heads_{d}"], 3) for d in ("fwd", "bwd")},
                         "slices_bit_equal": same,
                         "scratch_bytes_per_slice": {"fwd": 4 * ast["partials"] * (D + 2), "bwd_delta": bst["delta_bytes"] // Z,
                                                     "bwd_rows": bst["row_scratch_bytes"] // Z,
                                                     "bwd_cols": bst["col_scratch_bytes"] // Z},
                         "attention_stats": ast})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
