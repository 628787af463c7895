#!/usr/bin/env python3
"""bench.py — SDDMM GFLOP/s (2*nnz*K) of the BSMR engine on MI355X, reference headline metric.

Default (the driver's line): step = one SDDMM pass (one launch: dense-tile MFMA + residual) over
the plan of the C2 workload of BASELINE.json: nips-like 1,500 x 12,419 pattern with 746,316 nnz
(the real nips.mtx is a missing blob of the reference), K = 128, fp32 A/B, alpha = delta = 0.3.
Reordering runs once before timing and is reported separately (the reference's GFLOP/s excludes it
too, Logger.hpp:178-180). Inputs are resident in HBM when the timed region starts.

A plain run (`bench.py --gpus 1 --steps K --warmup W`) does only that: plan, warm-up, the K timed
steps (stream launches, then the same K steps as one HIP graph: the line's value), the line.
`--dump-outputs DIR` also writes the last timed step's P to DIR/P.npy. `--full` adds every other
leg of the report after the timed steps: in-run PMC traffic and MFMA counters, cold steps, the
dense/residual split, the rocSPARSE and CPU baselines (N > 1: checkData of the gathered P and the
strong_C4 block). --config C1 is the CPU path's own line and is the same with or without --full.

Multi-GPU (python -m torch.distributed.run --nproc-per-node N bench.py --gpus N, or plain
`bench.py --gpus N`, which starts that launcher as a child process; a WORLD_SIZE other than
--gpus is an error, so the line's n_gpus is always --gpus): S sharded by
row panels (bsmr/dist.py); B is broadcast once from rank 0 over RCCL (xGMI), each
rank holds only its rows of A, and after timing P is gathered to rank 0 (bit-exact: each rank's
outputs compacted in plan order, or its contiguous CSR segment) and checked against the
product's host SDDMM (checkData rule). C2 (default) is weak scaling: the global pattern is N
copies of the nips-like pattern stacked vertically, copy b with its columns relabelled by a random
permutation (synth.stack_copies), so per-GPU work stays one C2; C3/C4/C5 are strong scaling of the
one matrix (C4 = the north_star reddit split). Two splits (--shard):
  * local (default): N contiguous original row panels of equal stored entries (for C2 exactly the
    copies); each rank builds the BSMR plan of its own panel and runs bsmr_sddmm on it.
  * global: row-panel shards of ONE global BSMR plan. Rank 0 builds the plan and broadcasts its row
    stage (the clustering result) over RCCL; every rank rebuilds the column stage from it, cuts the
    same contiguous panel ranges, uploads its panels' A rows and runs bsmr_sddmm_panels_local.
  Local is faster for both scalings (one-GPU rehearsal, tools/shard_sim.py, slowest of 8 shards:
  C2 copies 11.8 vs 13.5 us, reddit-like x1 0.600 vs 0.726 ms; see main_sharded_local).
No collective in the timed loop; value = all ranks' flops / the slowest rank's time.

Other BASELINE.json configs (extra measurements, not the driver's line): --config C3 (cop20k-like,
fp16, K=256), C4 (reddit-like power-law graph, fp32, K=128; --scale shrinks it), C5 (DLMC-like
2048^2 90 % sparse mask, bf16, K=512; --mask uniform|block).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "sddmm-gpu_amd"))

METRIC = "SDDMM GFLOP/s (2·nnz·K) + HBM GB/s %peak, K=128, 1/2/4/8 MI355X"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip table (spec)
MFMA_HALF_PEAK_TFS = 2500.0  # MI355X_MICROARCH.md: BF16/FP16 MFMA ~2.5 PF dense


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="C2", choices=["C1", "C2", "C3", "C4", "C5"],
                    help="BASELINE.json config (C1 = the OpenMP host path on nips-like K = 32: its "
                         "line is the CPU leg timed until steady, with the GPU's run of the same "
                         "workload and their checkData beside it, with or without --full; "
                         "--steps and --warmup there set the GPU leg's steps only)")
    ap.add_argument("--K", type=int, default=None)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--delta", type=float, default=0.3)
    ap.add_argument("--scale", type=float, default=1.0, help="C4 size factor")
    ap.add_argument("--mask", default="uniform", choices=["uniform", "block"], help="C5 mask")
    ap.add_argument("--layout", default="auto", choices=["auto", "rowblock", "colmajor"],
                    help="SDDMM launch layout (bsmr_plan_options.layout)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg of the report: the "
                         "in-run PMC passes (roofline.traffic, mfma.busy), the cold steps, the "
                         "dense/residual split launches, the forced-MFMA split, the rocSPARSE and "
                         "CPU baselines; multi-GPU: the checkData of the gathered P and the "
                         "strong_C4 block. Off by default: a plain run sets up, warms up, times "
                         "the steps and prints the line. The --no-* / --pmc / --cold-steps "
                         "options below trim a --full run")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write the P of the last timed step as DIR/P.npy "
                         "(float32, CSR order; outputs over 64 MB: a fixed seeded sample of the "
                         "entries). Inputs are the same from run to run, so two builds can be "
                         "compared output for output")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-vendor", action="store_true",
                    help="skip the rocSPARSE SDDMM baseline leg (vendor_baseline)")
    ap.add_argument("--no-split", action="store_true",
                    help="skip the cold steps and the dense/residual split launches (rocprof runs: "
                         "every traced launch of the kernel is then a timed-region step)")
    ap.add_argument("--traffic-json", default=None,
                    help="PMC summary with hbm_bytes_per_launch for roofline.traffic (default: "
                         "profiles/traffic_<config>_K<K>.json when present)")
    ap.add_argument("--pmc", default="auto", choices=["auto", "on", "off"],
                    help="roofline.traffic measured in this run: two rocprofv3 PMC passes "
                         "(FETCH_SIZE, WRITE_SIZE) over tools/prof_sddmm.py on the same workload, "
                         "run as child processes before this process touches the GPU (auto: at "
                         "N=1 when rocprofv3 is on PATH)")
    ap.add_argument("--shard", default="auto", choices=["auto", "global", "local"],
                    help="multi-GPU split: global = row-panel shards of one global BSMR plan "
                         "(rank 0 clusters, row stage broadcast); local = contiguous original row "
                         "panels of S balanced by stored entries, each rank clustering its own "
                         "panel; auto = local (measured faster for C2 and C4: DESIGN.md section 7)")
    ap.add_argument("--force-sharded", action="store_true",
                    help="run the multi-GPU path (torch.distributed, RCCL) even at world size 1")
    ap.add_argument("--strong", default="auto", choices=["auto", "on", "off"],
                    help="strong_C4 block (the north_star reddit row-panel split, both splits, "
                         "with the global plan's N = 1 point); auto = for C2 at N > 1 under --full")
    ap.add_argument("--rebalance", type=int, default=2,
                    help="global split: rounds of measured-cost re-cutting "
                         "(bsmr_plan_shard_rebalance) before the timed steps")
    ap.add_argument("--strong-scale", type=float, default=1.0,
                    help="reddit-like size of the strong_C4 block (1 = 232 M stored entries)")
    ap.add_argument("--no-graph", action="store_true",
                    help="time the steps as stream launches only (default: the K timed steps "
                         "captured into one HIP graph and replayed; both are reported)")
    ap.add_argument("--sustained", action="store_true",
                    help="also time the K-step graph after ~40 ms of back-to-back replays (the "
                         "busy-device figure, timing.sustained_*; information only)")
    ap.add_argument("--cold-steps", type=int, default=20,
                    help="steps timed after evicting the 256 MiB Infinity Cache (0 = skip)")
    return ap.parse_args()


def workload(args):
    from bsmr import F16, F32, BF16, synth

    if args.config == "C2":
        M, N, rp, ci = synth.nips_like()
        return (M, N, rp, ci), args.K or 128, F32, (
            "C2: nips_like 1500x12419, 746,316 nnz (Zipf 1.1 columns, seed 20250801), fp32 A/B")
    if args.config == "C3":
        return synth.cop20k_like(), args.K or 256, F16, (
            "C3: cop20k_A_like 121192^2 FEM band+random (seed 20250802), fp16 A/B, fp32 accumulate")
    if args.config == "C4":
        return synth.reddit_like(args.scale), args.K or 128, F32, (
            f"C4: reddit_like Chung-Lu power law x{args.scale} (seed 20250803), fp32 A/B")
    return synth.dlmc_like(args.mask), args.K or 512, BF16, (
        f"C5: dlmc_like 2048^2 90% sparse {args.mask} mask (seed 7), bf16 A/B, fp32 accumulate")


DUMP_MAX_BYTES = 64 << 20  # --dump-outputs: everything written stays under this
DUMP_SAMPLE_SEED = 20250804


def dump_outputs(path, P):
    """--dump-outputs: P of the last timed step as <path>/P.npy (float32, CSR order of the stored
    entries). A P over DUMP_MAX_BYTES is written as a fixed sample: the entries at
    sorted(default_rng(DUMP_SAMPLE_SEED).integers(0, nnz, n)), the same positions in every run."""
    import numpy as np

    P = np.ascontiguousarray(P, np.float32).reshape(-1)
    n = (DUMP_MAX_BYTES - 4096) // 4  # room for the .npy header
    if P.size > n:
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).integers(0, P.size, n))
        P = P[idx]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "P.npy"), P)


# the CPUs this process may run on, read at start-up (an OpenMP runtime started with
# OMP_PROC_BIND would bind the main thread to one place, and sched_getaffinity of the main thread
# would no longer show the process's share)
AFFINITY = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))
AFFINITY_CPUS = len(AFFINITY)


def host_threads():
    """Host threads for the CPU legs (OMP_NUM_THREADS = nproc): OMP_NUM_THREADS
    when the environment sets it — a GPU box exports its CPU share there (16 per GPU) — else
    every CPU this process may run on (its start-up affinity mask), never more than that mask."""
    n = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or AFFINITY_CPUS
    return max(1, min(n, AFFINITY_CPUS))


def close_cpus(threads):
    """BASELINE.md §2's OMP_PROC_BIND=close for the CPU leg's `threads` OpenMP threads: one per
    physical core where the affinity set lists SMT siblings (Linux numbers them core, core + cores),
    in order — the CPUs the oracle pins its team to (orc_sddmm_cpu_rows_bound), so only this team is
    bound whatever OpenMP runtime the process started first."""
    cores = []
    try:
        sib = {}
        for c in AFFINITY:
            with open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list") as f:
                sib[c] = f.read().strip()
        seen = set()
        for c in AFFINITY:
            if sib[c] not in seen:
                seen.add(sib[c])
                cores.append(c)
    except OSError:
        cores = list(AFFINITY)
    return (cores + [c for c in AFFINITY if c not in cores])[:max(1, threads)]


def host_cpu_info(threads):
    """What the CPU leg ran on (core count, binding, CPU model)."""
    return {"threads": threads, "nproc": os.cpu_count(), "affinity_cpus": AFFINITY_CPUS,
            "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS"),
            "OMP_PROC_BIND": os.environ.get("OMP_PROC_BIND"), "model": cpu_model()}


def steady_runs(fn, budget_s=20.0, window=5, tol=0.05, max_runs=200, max_budget_s=75.0,
                drift_tol=0.03):
    """Time fn() until steady, or until the time budget ends (at least `window` runs either way).
    Steady: the last `window` runs agree within `tol` (max / min - 1), or — runs that scatter
    more than that on a shared host (C4 x1: 2.6-3.1 s per run at 16 threads) — the median of the
    last window is within `drift_tol` of the median of the window before it (no drift left, only
    run-to-run noise). Returns (median of the last window in s, every run's seconds, the criterion
    that held: "window", "no drift" or None). The first runs of a host loop on a fresh box fall
    steadily (page faults, frequency ramp: 3.1 -> 0.9 ms over 50 runs of C1 in round 3), so a
    median over all runs mixes the warm-up drift into the figure. Long runs (C4 x1: ~3 s) get room
    for 20 of them: budget max(budget_s, 20 x the first run), at most max_budget_s."""
    times = []
    t0 = time.perf_counter()
    fn()
    times.append(time.perf_counter() - t0)
    t_end = t0 + min(max_budget_s, max(budget_s, 20.0 * times[0]))
    while True:
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
        last = times[-window:]
        ok = None
        if len(times) >= window and max(last) <= (1.0 + tol) * min(last):
            ok = "window"
        elif len(times) >= 2 * window:
            m1, m0 = statistics.median(last), statistics.median(times[-2 * window:-window])
            if abs(m1 - m0) <= drift_tol * m1:
                ok = "no drift"
        if ok or len(times) >= max_runs or (len(times) >= window and time.perf_counter() > t_end):
            return statistics.median(last), times, ok


GRAPH_LEAD_CYCLES = 200_000  # torch.cuda._sleep spin ahead of each timed replay (~0.1 ms)


def graph_time(launch, steps, dev, out=None, reps=3):
    """ms per step of `steps` launches captured into one HIP graph and replayed (one warm-up
    replay, then `reps` timed replays, each between HIP events on the replay stream; the median).
    launch(stream_handle) issues one step on the given stream. A graph replay submits the K
    kernels without a host call per launch (the MI355X-native form of a launch-bound loop; at
    ~10 us per C2 step the ctypes + hipLaunchKernel path per step is as long as the kernel).
    out: the output tensor the steps write; it is zeroed after the warm-up replay, one more
    untimed replay fills it, and that P is returned, so the caller can check that the replayed
    graph computed the same P. Returns (ms, None, P or None, [ms per replay]), or (None, reason, None, []) when
    capture fails (the caller then keeps the stream-launched time)."""
    import torch

    try:
        gs = torch.cuda.Stream(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(gs):
            with torch.cuda.graph(g, stream=gs):
                for _ in range(steps):
                    launch(gs.cuda_stream)
            g.replay()  # warm-up replay
            gs.synchronize()
            P = None
            if out is not None:
                # P zeroed, one more (untimed) replay, and its P kept for the caller's check: the
                # replayed graph must write every output
                out.zero_()
                g.replay()
                gs.synchronize()
                P = out.cpu().numpy().copy()
            times = []
            for r in range(max(1, reps)):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                # a short spin kernel queued ahead of the start event keeps the stream busy while
                # the host submits the event and the graph, so the events bracket the K steps'
                # device time and not the host's graph-launch latency (≈ 10 µs per replay, 0.5 µs
                # per step at the driver's 20 steps; rocprofv3 trace of the driver's command,
                # DESIGN.md §8). The steps themselves are unchanged.
                torch.cuda._sleep(GRAPH_LEAD_CYCLES)
                e0.record(gs)
                g.replay()
                e1.record(gs)
                gs.synchronize()
                times.append(e0.elapsed_time(e1) / max(steps, 1))
        del g
        return statistics.median(times), None, P, times
    except Exception as e:  # noqa: BLE001 - reported; the stream-launched time stays
        torch.cuda.synchronize()
        return None, f"{type(e).__name__}: {e}"[:300], None, []


def sustained_time(launch, steps, dev, warm_ms=40.0, reps=10):
    """ms per step of the same K-step graph once the device has run it back to back for warm_ms
    (the clocks and memory-side state of a busy GPU; the line's `value` is timed from the
    standing start the driver's command gives). Reported beside `value`, never as it:
    (ms, [ms per timed replay]) or (None, reason)."""
    import torch

    try:
        gs = torch.cuda.Stream(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(gs):
            with torch.cuda.graph(g, stream=gs):
                for _ in range(steps):
                    launch(gs.cuda_stream)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(gs)
            g.replay()
            e1.record(gs)
            gs.synchronize()
            n = max(1, int(warm_ms / max(e0.elapsed_time(e1), 1e-3)))
            for _ in range(n):  # back to back, no host wait between replays
                g.replay()
            times = []
            evs = []
            for _ in range(reps):
                a0 = torch.cuda.Event(enable_timing=True)
                a1 = torch.cuda.Event(enable_timing=True)
                a0.record(gs)
                g.replay()
                a1.record(gs)
                evs.append((a0, a1))
            gs.synchronize()
            times = [a.elapsed_time(b) / max(steps, 1) for a, b in evs]
        del g
        return statistics.median(times), times
    except Exception as e:  # noqa: BLE001 - reported only
        torch.cuda.synchronize()
        return None, f"{type(e).__name__}: {e}"[:300]


def cpu_baseline(M, N, rp, ci, K, A, B, P_gpu):
    """Oracle host SDDMM (host.cpp:45-76 restated), timed on this box's host cores over the whole
    workload (C4 x1: 59 GFLOP per run, about 0.6 s at 16 threads) until steady."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np

    import oracle_lib as O

    threads = host_threads()
    c = O.CSR.from_arrays(M, N, rp, ci)
    lib = O.lib()
    Af = np.ascontiguousarray(A, np.float32)
    Bf = np.ascontiguousarray(B, np.float32)
    # bounded sample: whole rows from the start, at most 100 GFLOP per run (every BASELINE config
    # runs whole: C4 x1 is 59 GFLOP)
    budget = 1e11
    row_end, acc = M, 0.0
    for r in range(M):
        acc += 2.0 * (int(rp[r + 1]) - int(rp[r])) * K
        if acc >= budget:
            row_end = r + 1
            break
    nnz_s = int(rp[row_end])
    P = np.empty(len(ci), np.float32)
    cpus = np.asarray(close_cpus(threads), np.int32)
    pinned = []
    med, times, ok = steady_runs(lambda: pinned.append(lib.orc_sddmm_cpu_rows_bound(
        c.h, K, Af, Bf, P, 0, row_end, threads, cpus.ctypes.data, len(cpus))))
    nerr = O.check_data(P[:nnz_s], P_gpu[:nnz_s])
    model = cpu_model()
    full = "full workload" if row_end == M else f"rows [0, {row_end}) of {M}"
    return {
        "value": round(2.0 * nnz_s * K / med / 1e9, 3),
        "unit": "GFLOP/s",
        "cores": threads,
        "kind": "port",
        "sample": f"{full} (nnz={nnz_s}, K={K}), median of the last 5 of {len(times)} runs "
                  f"({'within 5 %' if ok == 'window' else 'its median within 3 % of the 5 before (no drift; runs scatter more than 5 % on this host)' if ok else 'time budget reached before the runs were steady'}), "
                  f"OpenMP over rows, threads pinned close, one per core (oracle/oracle.cpp "
                  f"orc_sddmm_cpu_rows_bound); cpu: {model}",
        "ms": round(med * 1e3, 3),
        "steady": bool(ok),
        "steady_criterion": ok,
        "runs_ms": [round(t * 1e3, 3) for t in times],
        "host": dict(host_cpu_info(threads), bind="close (explicit)", cpus=[int(x) for x in cpus],
                     threads_pinned=min(pinned) if pinned else 0),
        "checkData_errors_vs_gpu": nerr,
    }


def rowblock_bounds(st, rby, ms):
    """The row-block kernel's on-chip traffic per launch against the rates that bound it
    (MI355X_MICROARCH.md, measured): L2 -> CU ingest (A row blocks staged once per item, one B row
    per column-run piece, 8 B of metadata per entry and per piece, a B tile per MFMA tile) at
    16.8-18.8 TB/s chip-wide for gathered rows served from L2, and LDS reads (one A row per
    residual entry, 16 A rows per tile) at ~150 TB/s (ds_read_b128, every CU streaming)."""
    i = {128: 0, 256: 1, 512: 2, 1024: 3, 2048: 4}[rby]
    rows, items, pieces = st["rb_rows"][i], st["rb_work_items"][i], st["rb_pieces"][i]
    entries, tiles = st["rb_entries"][i], st["rb_tiles"][i]
    ingest = items * rows * rby + pieces * rby + 8.0 * (entries + pieces) + tiles * 16 * rby
    lds = entries * rby + tiles * 16 * rby
    t = ms * 1e-3
    return {
        "l2_to_cu": {"bytes": ingest, "achieved_TBps": round(ingest / t / 1e12, 2),
                     "ref_TBps": 17.8, "frac": round(ingest / t / 17.8e12, 3)},
        "lds_read": {"bytes": lds, "achieved_TBps": round(lds / t / 1e12, 2),
                     "ref_TBps": 150.0, "frac": round(lds / t / 150e12, 3)},
        "layout": {"rows_per_block": rows, "items": items, "pieces": pieces,
                   "entries": entries, "mfma_tiles": tiles},
    }


def mfma_report(st, st_after, nnz, rby, dtiles, kern, no_tiles, measured=None):
    """MFMA use of the timed launch (BASELINE.md §3 per-config fields). SURVEY.md §8d's MFMA
    efficiency = 2·nnz_dense·K / (256·2·K·#denseBlocks): stored entries per 16 x 16 output slot of
    the tiles computed on the matrix cores, for the BSMR plan's tiles (the reference's dense
    blocks) and for the tiles this launch actually put on MFMA."""
    ntiles = st["num_dense_tiles"]
    r = {"efficiency_definition": "stored entries per output slot of the MFMA tiles "
                                  "(SURVEY.md §8d: 2 nnz_dense K / (256 * 2 K * #denseBlocks))",
         "bsmr_plan_tiles": {"tiles": ntiles, "entries": nnz - st["num_residual"],
                             "efficiency": round((nnz - st["num_residual"]) / (256.0 * ntiles), 4)
                             if ntiles else None}}
    if kern.startswith("k_sddmm_ptile"):
        r["launch"] = {"kind": "panel-grouped BSMR 16 x 16 tiles, every tile on MFMA", "tiles": ntiles,
                       "efficiency": r["bsmr_plan_tiles"]["efficiency"]}
    elif dtiles:
        r["launch"] = {"kind": "dense-sampled 128 x 128 tiles", "tiles": dtiles,
                       "efficiency": round(nnz / (16384.0 * dtiles), 4)}
    elif kern.startswith("k_sddmm_rb"):
        i = {128: 0, 256: 1, 512: 2, 1024: 3, 2048: 4}[rby]
        kept = st_after["rb_tiles"][i]
        r["launch"] = {"kind": "row-block launch, kept 16 x 16 tiles", "tiles": kept,
                       "efficiency": round((nnz - st_after["rb_entries"][i]) / (256.0 * kept), 4)
                       if kept else None}
        if no_tiles:
            r["busy_note"] = ("no MFMA instruction in this launch: every tile's entries run as "
                              "residual entries on the vector ALUs (fp32 MFMA runs at the vector "
                              "FMA rate on gfx950; half tiles under 128 entries are demoted)")
    if measured:  # the in-run PMC pass (mfma_busy)
        r.update(measured)
    elif no_tiles:
        r["busy"] = 0.0
        r["busy_source"] = "by construction (no MFMA instruction; no PMC pass in this run)"
    return r


def forced_mfma_split(args, pattern, K, dtype, dA, dB, dev, stream, P_ref, flops):
    """The config's dense-tile vs residual split when the default layout keeps no MFMA tile: the
    same pattern planned with every BSMR tile kept on the matrix cores (tile_min = 0, reordered
    row blocks), its fused
    launch timed like the line's steps, then its dense-tile-only and residual-only launches
    (bsmr_sddmm_profile) — the reference times its two streams separately
    (sddmmKernel.cu:2555-2659). P is checked against the line's P."""
    import torch

    from bsmr import F32, Plan, check_data

    M, N, rp, ci = pattern
    tun = dict(args.tuning or {})
    tun["tile_min_f32" if dtype == F32 else "tile_min_half"] = 0
    tun["orig_rows"] = 0  # original-order row blocks carry no tiles (every entry residual)
    plan = Plan(M, N, rp, ci, alpha=args.alpha, delta=args.delta, device=dev.index,
                layout=args.layout, tuning=tun)
    dP = torch.zeros(len(ci), dtype=torch.float32, device=dev)
    sp = stream.cuda_stream

    def step():
        plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), stream=sp, dtype=dtype)

    for _ in range(max(3, args.warmup)):
        step()
    torch.cuda.synchronize()
    n = max(10, min(args.steps, 100))
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(n):
        step()
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    prof = plan.profile(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), iters=20, stream=sp,
                        dtype=dtype)
    st = plan.stats()
    i = {128: 0, 256: 1, 512: 2, 1024: 3, 2048: 4}.get(K * (4 if dtype == F32 else 2))
    out = {"tuning": tun, "ms_per_step": round(ms, 5),
           "value": round(flops / (ms * 1e-3) / 1e9, 2),
           "kernels_ms": {k: round(v, 5) for k, v in prof.items()},
           "checkData_errors_vs_line": check_data(P_ref, dP.cpu().numpy())}
    if i is not None:
        kept = st["rb_tiles"][i]
        out["mfma_tiles"] = kept
        out["entries_on_mfma"] = len(ci) - st["rb_entries"][i] if st["rb_rows"][i] else None
    del plan, dP
    return out


def vendor_baseline(M, N, K, rp, ci, dA, dB, P_engine, dtype, stream, flops, engine_ms):
    """rocsparse_sddmm on the same device operands (the reference's cuSPARSE baseline,
    include/cuSparseSDDMM.cuh:27-145): preprocess once, then timed back-to-back calls, for the
    default algorithm (the reference's CUSPARSE_SDDMM_ALG_DEFAULT) and rocSPARSE's dense one."""
    import numpy as np
    import torch

    from bsmr import BsmrError, check_data
    from bsmr.vendor import RocsparseSddmm

    dev = dA.device
    d_rp = torch.from_numpy(rp.astype(np.int32)).to(dev)
    d_ci = torch.from_numpy(ci.astype(np.int32)).to(dev)
    sp = stream.cuda_stream
    out = {"name": "rocsparse_sddmm (CSR i32, fp32 compute, alpha 1, beta 0)", "unit": "GFLOP/s"}
    best = None
    for alg in ("default", "dense"):
        if alg == "dense" and 4.0 * M * N > 4e9:  # alg_dense materialises C as M x N fp32
            out[alg] = {"skipped": f"dense C would take {4.0 * M * N / 1e9:.0f} GB"}
            continue
        try:
            rs = RocsparseSddmm(M, N, K, len(ci), d_rp.data_ptr(), d_ci.data_ptr(), dtype=dtype,
                                alg=alg, stream=sp)
        except BsmrError as e:  # e.g. bf16 operands in this rocSPARSE build
            out[alg] = {"error": str(e)}
            continue
        dP = torch.zeros(len(ci), dtype=torch.float32, device=dev)  # read even with beta = 0

        def call():
            rs(dA.data_ptr(), dB.data_ptr(), dP.data_ptr())

        try:
            call()
        except BsmrError as e:
            out[alg] = {"error": str(e)[-400:]}
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        one = time.perf_counter() - t0
        iters = max(3, min(100, int(2.0 / max(one, 1e-6))))
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            call()
        e1.record(stream)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        r = {"value": round(flops / (ms * 1e-3) / 1e9, 2), "ms": round(ms, 5), "iters": iters,
             "checkData_errors_vs_engine": check_data(dP.cpu().numpy(), P_engine)}
        out[alg] = r
        del rs, dP
        if r["checkData_errors_vs_engine"] == 0 and (best is None or ms < best[1]):
            best = (alg, ms, r["value"])
    if best is not None:
        out.update({"value": best[2], "ms": round(best[1], 5), "best_alg": best[0],
                    "engine_speedup": round(best[1] / engine_ms, 2)})
    return out


def kernel_name(st, st_after, K, dtype, layout):
    """The launch bsmr_sddmm picks (sddmm.hip rb_slot / launch_half / use_dense)."""
    from bsmr import F32

    rby = K * (4 if dtype == F32 else 2)
    if st_after.get("ptile_items"):  # sddmm.hip use_ptile (its item list is built on first use)
        return (f"k_sddmm_ptile<{'f16' if dtype == 1 else 'bf16'},{K // 32}> (panel-grouped BSMR "
                f"tiles, every tile on MFMA 16x16x32: equal tile runs, one per CU, their panels' A "
                f"rows staged in LDS once, {st_after['ptile_items']} item slots; residual in "
                f"column-major slots)"), rby
    tile_dominated = st["num_residual"] * 4 < st["num_dense_tiles"] * 16  # sddmm.hip rb_slot
    if rby in (128, 256, 512, 1024, 2048) and layout != "colmajor" and not tile_dominated:
        tiles = ("fp32 tiles demoted to residual entries" if dtype == F32
                 else "dense-tile MFMA for tiles >= 128 entries")
        i = {128: 0, 256: 1, 512: 2, 1024: 3, 2048: 4}[rby]
        rows = st_after["rb_rows"][i]
        nt = 1024 if rby * rows > 80 * 1024 else 512
        # sddmm.hip launch_rb: staged output (P > 8 MiB) by runs, no kept MFMA tile, rows of
        # >= 512 bytes, >= 4096 items -> the pair kernel (two list positions per workgroup)
        pair = (4 * st["nnz"] > (8 << 20) and rby >= 512 and st_after["rb_items"][i] >= 4096
                and not st_after["rb_tiles"][i])
        name = "k_sddmm_rb_pair" if pair else "k_sddmm_rb"
        # template arguments as rocprofv3 prints them: <dtype, row bytes, threads, dynamic piece
        # batches, lean single-item form (no kept tiles, direct stores; sddmm.hip launch_rb)>
        dyn = bool(st_after.get("rb_batches", 0) & (1 << i))
        lite = not pair and 4 * st["nnz"] <= (8 << 20) and not st_after["rb_tiles"][i]
        targs = f"{dtype},{rby},{nt},{str(dyn).lower()}" + ("" if pair else f",{str(lite).lower()}")
        return (f"{name}<{targs}> (row-block LDS layout, {rby}-byte rows, {rows} "
                f"rows per block: residual entries; {tiles}"
                f"{'; staged output by runs, two items per workgroup' if pair else ''}"
                f"{'; lean single-item kernel' if lite else ''})"), rby
    if dtype == F32:
        return f"k_sddmm_f32<{K}> (column-major slots: dense-tile MFMA + residual)", rby
    return f"k_sddmm_half<{'f16' if dtype == 1 else 'bf16'}> (dense-tile MFMA + residual)", rby


def traffic_for(args, K):
    """roofline.traffic fallback: HBM bytes per launch from a committed PMC summary of this config
    (tools/pmc_traffic.py), used only if it was measured on the kernel sources of this tree (their
    sha256 is recorded in the file); None otherwise. Candidates: --traffic-json, else
    profiles/traffic_<config>_K<K>.json and profiles/*/<label>/traffic.json (label C2, C3, C4,
    C5u, C5b), newest round first."""
    import glob
    import hashlib

    label = args.config + ({"uniform": "u", "block": "b"}[args.mask] if args.config == "C5" else "")
    if args.traffic_json:
        cands = [args.traffic_json]
    else:
        cands = [os.path.join(ROOT, "profiles", f"traffic_{args.config}_K{K}.json")]
        cands += sorted(glob.glob(os.path.join(ROOT, "profiles", "*", label, "traffic.json")),
                        reverse=True)
    last = None
    for tj in cands:
        if not os.path.exists(tj):
            continue
        with open(tj) as f:
            t = json.load(f)
        srcs = t.get("kernel_sources_sha256")
        if not srcs:
            last = {"file": os.path.relpath(tj, ROOT), "status": "no source hash: not used"}
            continue
        stale = None
        for rel, h in srcs.items():
            with open(os.path.join(ROOT, rel), "rb") as f:
                if hashlib.sha256(f.read()).hexdigest() != h:
                    stale = rel
                    break
        if stale:
            last = {"file": os.path.relpath(tj, ROOT), "status": f"stale: {stale} changed since the PMC run"}
            continue
        return t.get("hbm_bytes_per_launch"), {"file": os.path.relpath(tj, ROOT),
                                               "measured_on": t.get("measured_on"),
                                               "status": "kernel sources match"}
    return None, last


def pmc_traffic_inrun(args):
    """roofline.traffic measured now: HBM bytes per launch of the fused SDDMM kernel on this
    workload, from two rocprofv3 PMC passes (one counter each: FETCH_SIZE needs 3 of the 4 TCC
    counters, WRITE_SIZE 2) over tools/prof_sddmm.py, corrected as MI355X_MICROARCH.md's HBM
    section prescribes (FETCH_SIZE KiB x 2 on gfx950, WRITE_SIZE KiB as reported). The children
    run before this process initialises the GPU. Returns (bytes or None, source dict)."""
    import shutil
    import subprocess
    import tempfile

    if args.pmc == "off":
        return None, {"status": "--pmc off"}
    rp = shutil.which("rocprofv3")
    if not rp:
        return None, {"status": "rocprofv3 not on PATH"}
    wl = {"C2": ["--workload", "nips_like", "--dtype", "f32"],
          "C3": ["--workload", "cop20k_like", "--dtype", "f16"],
          "C4": ["--workload", "reddit_like", "--scale", str(args.scale), "--dtype", "f32"],
          "C5": ["--workload", "dlmc_like", "--mask", args.mask, "--dtype", "bf16"]}[args.config]
    K = args.K or {"C2": 128, "C3": 256, "C4": 128, "C5": 512}[args.config]
    wl += ["--K", str(K), "--layout", args.layout, "--iters", "5"]
    tmp = tempfile.mkdtemp(prefix="bench_pmc_", dir="/tmp")
    limit = 600 if args.config == "C4" else 180
    t0 = time.perf_counter()
    # three passes, one counter group each (FETCH_SIZE takes 3 of the 4 TCC counters, WRITE_SIZE
    # 2; the MFMA group is 6 SQ + 1 GRBM counters)
    for name, ctr in (("fetch", ["FETCH_SIZE"]), ("write", ["WRITE_SIZE"]), ("mfma", MFMA_PMC)):
        cmd = ["timeout", "-s", "KILL", str(limit), rp, "--pmc"] + ctr + ["--kernel-include-regex",
               "k_sddmm", "--output-format", "csv", "-d", os.path.join(tmp, name), "-o", "run",
               "--", sys.executable, os.path.join(ROOT, "tools", "prof_sddmm.py")] + wl
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                           text=True)
        if r.returncode != 0:
            return None, {"status": f"rocprofv3 --pmc {ctr} failed (rc {r.returncode})",
                          "stderr_tail": r.stderr[-300:]}
    try:
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "pmc_table.py"),
                                       tmp], text=True)
        full = json.loads(out)["full"]
        fetch = 2.0 * full["FETCH_SIZE"] * 1024.0
        write = full["WRITE_SIZE"] * 1024.0
        mfma = {c: full.get(c) for c in MFMA_PMC}
    except (subprocess.CalledProcessError, KeyError, ValueError) as e:
        return None, {"status": f"PMC parse failed: {e}"}
    shutil.rmtree(tmp, ignore_errors=True)
    return round(fetch + write), {
        "status": "measured in this run", "fetch_bytes": round(fetch), "write_bytes": round(write),
        "method": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE / the MFMA group (separate passes) "
                  "over tools/prof_sddmm.py --iters 5, median over the fused launches; FETCH_SIZE "
                  "KiB x 2 (gfx950) + WRITE_SIZE KiB",
        "mfma_counters": mfma,
        "seconds": round(time.perf_counter() - t0, 1)}


# the MFMA counter pass of the in-run PMC (one run: 6 SQ + 1 GRBM counters)
MFMA_PMC = ["SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CU_CYCLES", "SQ_INSTS_VALU_MFMA_MOPS_BF16",
            "SQ_INSTS_VALU_MFMA_MOPS_F16", "SQ_INSTS_VALU_MFMA_MOPS_F32", "SQ_INSTS_MFMA",
            "GRBM_GUI_ACTIVE"]


def mfma_busy(counters, nnz, K):
    """MFMA use of the fused launch from its PMC pass (MI355X_MICROARCH.md: SQ_VALU_MFMA_BUSY_CYCLES
    counts matrix-pipe cycles summed over SIMDs; GRBM_GUI_ACTIVE is summed over the 8 XCDs, so the
    launch's wall cycles are / 8; 256 CUs x 4 SIMDs; one MFMA MOP = 512 flops)."""
    busy, grbm = counters.get("SQ_VALU_MFMA_BUSY_CYCLES"), counters.get("GRBM_GUI_ACTIVE")
    if busy is None or not grbm:
        return None
    mops = sum(counters.get(k) or 0.0 for k in MFMA_PMC if k.startswith("SQ_INSTS_VALU_MFMA_MOPS"))
    wall = grbm / 8.0
    r = {"busy": round(busy / (wall * 1024.0), 4),
         "busy_definition": "SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 1024 SIMDs): the "
                            "fraction of all SIMD cycles of the launch (under the PMC pass) the "
                            "matrix pipes were busy",
         "mfma_instructions": counters.get("SQ_INSTS_MFMA"),
         "mfma_flops": mops * 512.0,
         "source": "rocprofv3 --pmc pass in this run (fused launch, median)"}
    if mops:
        r["sampled_flops_per_mfma_flop"] = round(2.0 * nnz * K / (mops * 512.0), 4)
    if counters.get("SQ_BUSY_CU_CYCLES"):
        r["busy_of_cu_busy_cycles"] = round(busy / (4.0 * counters["SQ_BUSY_CU_CYCLES"]), 4)
    return r


def _free_port():
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(args):
    """`bench.py --gpus N` without a launcher (no WORLD_SIZE): start N ranks under
    torch.distributed.run as a CHILD process — this process never touches HIP, and nothing is
    exec'd — forward its output and exit with its return code. So `--gpus N` always means N ranks
    (one per GPU); rank 0 of the child prints the JSON line."""
    import subprocess

    if args.gpus < 1:
        print(f"bench.py: --gpus {args.gpus} must be >= 1", file=sys.stderr)
        return 2
    if os.environ.get("BSMR_DIST_BACKEND", "nccl") != "gloo":
        import torch  # device_count() does not initialise HIP

        n = torch.cuda.device_count()
        if n < args.gpus:
            print(f"bench.py: --gpus {args.gpus} but only {n} GPU(s) visible", file=sys.stderr)
            return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, BSMR_BENCH_SELF_LAUNCHED="1")
    print(f"bench.py: launching {args.gpus} rank(s): {' '.join(cmd)}", file=sys.stderr, flush=True)
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
    for line in p.stdout:  # rank 0's JSON line (and any progress) as it comes
        sys.stdout.write(line)
        sys.stdout.flush()
    return p.wait()


def main():
    args = parse()
    from bsmr import dist as D

    rank, world, local = D.env_rank_world()
    launched = "WORLD_SIZE" in os.environ
    if args.config != "C1":
        if launched and world != args.gpus:
            # the line's n_gpus must be the --gpus the caller asked for
            print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} "
                  "ranks", file=sys.stderr)
            return 2
        if not launched and (args.gpus > 1 or args.force_sharded):
            return self_launch(args)
    if os.environ.get("BSMR_BENCH_PROBE") == "1":  # launch-path test: report and stop (no GPU)
        # line and newline in one write: the ranks share the launcher's pipe, and a print() on an
        # unbuffered stdout writes them separately, so two ranks' lines could run together
        sys.stdout.write(json.dumps({"probe": True, "rank": rank, "world": world,
                                     "gpus": args.gpus, "self_launched":
                                     os.environ.get("BSMR_BENCH_SELF_LAUNCHED") == "1"}) + "\n")
        sys.stdout.flush()
        return 0
    from bsmr import set_default_tuning, tuning_from_env

    # launch-layout knobs from BSMR_* variables (A/B runs; the library itself reads no
    # environment), recorded in the line when any is set
    args.tuning = tuning_from_env()
    set_default_tuning(args.tuning)
    if args.config == "C1":
        return main_c1(args)
    sharded = world > 1 or args.force_sharded
    # in-run PMC traffic (--full: children, before this process touches the GPU; N=1 only)
    args.pmc_result = pmc_traffic_inrun(args) if args.full and not sharded else (None, None)
    import torch

    if sharded:
        # one rank per GPU; BSMR_DIST_BACKEND=gloo with more ranks than GPUs only rehearses the
        # multi-process path (ranks then share devices; their timings are not a measurement)
        torch.cuda.set_device(local % torch.cuda.device_count())
        D.init(os.environ.get("BSMR_DIST_BACKEND", "nccl"))  # nccl = RCCL over xGMI
        return main_sharded(args, rank, world)
    torch.cuda.set_device(0)
    return main_single(args)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return ""


def main_c1(args):
    """BASELINE.json C1: nips-like K = 32 fp32 through the OpenMP host path (the product's
    bsmr_sddmm_cpu, host.cpp:45-76 restated: per stored entry a serial fp32 sum in k order, rows
    split over all host threads), timed on this box's cores (runs repeated until the last 5 agree within 5 %, median of those 5),
    then checkData (checkData.hpp:44-79) of its P against the GPU engine's P on the same
    operands; the GPU's K = 32 rate on the same plan is reported beside it."""
    import numpy as np
    import torch

    from bsmr import Plan, check_data, make_data, sddmm_cpu, synth

    M, N, rp, ci = synth.nips_like()
    K = args.K or 32
    nnz = len(ci)
    threads = host_threads()
    A = make_data(M * K)
    B = make_data(N * K)
    res = {}

    def run_cpu():
        res["P"] = sddmm_cpu(M, N, rp, ci, K, A, B, threads=threads)

    med, times, steady = steady_runs(run_cpu)
    P_cpu = res["P"]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, P_cpu)
    cpu_ms = med * 1e3
    flops = 2.0 * nnz * K
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    plan = Plan(M, N, rp, ci, alpha=args.alpha, delta=args.delta, device=0, layout=args.layout)
    dA = torch.from_numpy(A).to(dev)
    dB = torch.from_numpy(B).to(dev)
    dP = torch.zeros(nnz, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    for _ in range(args.warmup):
        plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), stream=sp)
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.steps):
        plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), stream=sp)
    e1.record(stream)
    torch.cuda.synchronize()
    gpu_ms = e0.elapsed_time(e1) / args.steps
    nerr = check_data(P_cpu, dP.cpu().numpy())
    st = plan.stats()
    out = {
        "metric": METRIC,
        "value": round(flops / (cpu_ms * 1e-3) / 1e9, 3),
        "unit": "GFLOP/s",
        "n_gpus": 0,
        "steps": min(5, len(times)),
        "warmup": max(0, len(times) - 5),
        "ms_per_step": round(cpu_ms, 4),
        "higher_is_better": True,
        "scaling": "none",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "C1: nips_like 1500x12419, 746,316 nnz (Zipf 1.1 columns, seed "
                               f"20250801), fp32 A/B, K={K}: OpenMP host path + checkData",
                   "M": M, "N": N, "nnz": nnz, "K": K,
                   "parallelism": f"host: {threads} threads (bsmr_sddmm_cpu, rows split into "
                                  "equal-entry ranges)"},
        "cpu": {"cores": threads, "model": cpu_model(), "host": host_cpu_info(threads),
                "kind": "product host SDDMM "
                "(csrc/host_check.cpp, host.cpp:45-76 loop order, no FMA contraction)",
                "runs_ms": [round(t * 1e3, 4) for t in times], "steady": bool(steady), "steady_criterion": steady,
                "rule": "runs until the last 5 agree within 5 % or their median is within 3 % of the 5 before (budget max(20 s, 20 runs)); "
                        "value = median of the last 5"},
        "checkData_errors_cpu_vs_gpu": nerr,
        "gpu_same_workload": {"value": round(flops / (gpu_ms * 1e-3) / 1e9, 2),
                              "ms_per_step": round(gpu_ms, 5), "steps": args.steps,
                              "alpha": args.alpha, "delta": args.delta,
                              "kernel": kernel_name(st, plan.stats(), K, 0, args.layout)[0],
                              "speedup_over_cpu": round(cpu_ms / gpu_ms, 1)},
    }
    print(json.dumps(out), flush=True)


def main_single(args):
    import numpy as np  # noqa: F401
    import torch

    from bsmr import F32, Plan, make_data

    world = 1
    dev = torch.device("cuda", torch.cuda.current_device())

    (M, N, rp, ci), K, dtype, desc = workload(args)
    nnz = len(ci)
    t0 = time.perf_counter()
    plan = Plan(M, N, rp, ci, alpha=args.alpha, delta=args.delta, device=dev.index,
                layout=args.layout)
    plan_s = time.perf_counter() - t0
    st = plan.stats()

    tdt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dtype]
    A = make_data(M * K)  # Matrix<float>(M,K,row_major).makeData
    dA = torch.from_numpy(A).to(dev).to(tdt)
    B = make_data(N * K)  # Matrix<float>(K,N,col_major).makeData
    dB = torch.from_numpy(B).to(dev).to(tdt)
    dP = torch.zeros(nnz, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream

    def step():
        plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), stream=sp, dtype=dtype)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)  # HIP events on the launch stream
    for _ in range(args.steps):
        step()
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    ms_per_step = ms / args.steps

    stream_ms_per_step = ms_per_step
    # the timed steps as one HIP graph (graph_time): the line's value when capture works,
    # the stream-launched time beside it
    P_stream = dP.cpu().numpy().copy()
    graph_ms, graph_err, P_graph, graph_reps = (None, "--no-graph", None, []) if args.no_graph \
        else graph_time(lambda h: plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
                                             stream=h, dtype=dtype), args.steps, dev, out=dP)
    timing = {"method": "hip_graph" if graph_ms is not None else "stream_launches",
              "graph_ms_per_step": round(graph_ms, 5) if graph_ms is not None else None,
              "graph_replays_ms_per_step": [round(x, 5) for x in graph_reps],
              "stream_launch_ms_per_step": round(stream_ms_per_step, 5),
              "note": "value = the K timed steps captured into one HIP graph and replayed "
                      "between HIP events (each step a full SDDMM launch; the median of 3 timed "
                      "replays, each queued behind a short spin kernel so the events bracket the "
                      "steps' device time, not the host's graph launch); stream_launch = the same "
                      "K steps launched one by one from Python"}
    if P_graph is not None:
        # P was zeroed before the timed replays: the replayed graph must have written every
        # output, bit-identical to the stream-launched steps (same kernel, same inputs)
        import numpy as np

        mism = int(np.count_nonzero(P_graph.view(np.uint32) != P_stream.view(np.uint32)))
        timing["graph_P_mismatches_vs_stream"] = mism
        if mism:
            timing["graph_error"] = f"replayed graph P differs from the stream-launched P in {mism} entries"
            graph_ms = None
            timing["method"] = "stream_launches"
    if graph_ms is not None:
        ms_per_step = graph_ms
    if graph_ms is not None and args.sustained:
        # the same K steps on a busy device (information only: the line's value stays the
        # standing-start figure above; opt-in, so a rocprofv3 summary of the default command
        # averages the same launches as the value)
        sus_ms, sus_reps = sustained_time(lambda h: plan.sddmm(dA.data_ptr(), dB.data_ptr(), K,
                                                               dP.data_ptr(), stream=h, dtype=dtype),
                                          args.steps, dev)
        if sus_ms is not None:
            timing["sustained_ms_per_step"] = round(sus_ms, 5)
            timing["sustained_replays_ms_per_step"] = [round(x, 5) for x in sus_reps]
            timing["sustained_value"] = round(2.0 * nnz * K / (sus_ms * 1e-3) / 1e9, 2)
            timing["sustained_note"] = ("the same K-step graph after ~40 ms of back-to-back replays "
                                        "(busy-device clocks; not the line's value)")
        else:
            timing["sustained_error"] = sus_reps
    if graph_err:
        timing["graph_error"] = graph_err
    if args.dump_outputs:  # dP holds the last timed step's P (the last replay's, or the stream's)
        torch.cuda.synchronize()
        dump_outputs(args.dump_outputs, dP.cpu().numpy())

    # everything below the timed steps is a leg of --full
    split = args.full and not args.no_split
    # cold: before each step a 512 MiB write evicts the Infinity Cache (MALL) and the L2s, so
    # A, B and the plan come from HBM; only the SDDMM launch is inside the events
    cold_ms = cold_clean_ms = None
    if args.cold_steps > 0 and split:
        junk = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        evs = []
        for i in range(args.cold_steps):
            junk.fill_(i & 0xFF)
            a0 = torch.cuda.Event(enable_timing=True)
            a1 = torch.cuda.Event(enable_timing=True)
            a0.record(stream)
            step()
            a1.record(stream)
            evs.append((a0, a1))
        torch.cuda.synchronize()
        cold_ms = statistics.median(a.elapsed_time(b) for a, b in evs)
        # the same with clean caches: the eviction reads 512 MiB instead of writing it, so the
        # launch does not also pay for writing back the dirty lines the write left in the L2s and
        # the MALL (two untimed read passes first turn the write leg's dirty lines clean)
        sink = torch.empty((), dtype=torch.int64, device=dev)
        for _ in range(2):
            sink.copy_(junk.sum(dtype=torch.int64))
        evs = []
        for i in range(args.cold_steps):
            sink.copy_(junk.sum(dtype=torch.int64))
            a0 = torch.cuda.Event(enable_timing=True)
            a1 = torch.cuda.Event(enable_timing=True)
            a0.record(stream)
            step()
            a1.record(stream)
            evs.append((a0, a1))
        torch.cuda.synchronize()
        cold_clean_ms = statistics.median(a.elapsed_time(b) for a, b in evs)
        del junk, sink

    # the same kernel split into its dense-tile-only and residual-only launches
    prof = {} if not split else plan.profile(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
                                             iters=20, stream=sp, dtype=dtype)
    P_gpu = dP.cpu().numpy() if args.full else None  # the baselines' checkData operand
    st_after = plan.stats()  # the launch layout is built on the first SDDMM call

    s = 4 if dtype == F32 else 2
    flops_rank = 2.0 * nnz * K
    value = flops_rank * world / (ms_per_step * 1e-3) / 1e9
    bytes_alg = s * K * (M + N) + 4.0 * nnz + 4.0 * (M + 1) + 4.0 * nnz
    achieved = bytes_alg / (ms_per_step * 1e-3) / 1e9
    traffic, traffic_src = args.pmc_result
    if traffic is None and args.full:  # a committed PMC summary measured on these kernel sources, if any
        t2, src2 = traffic_for(args, K)
        if t2 is not None:
            traffic, traffic_src = t2, dict(src2, inrun=traffic_src)
        elif traffic_src is not None and src2 is not None:
            traffic_src = dict(traffic_src, committed=src2)

    kern, rby = kernel_name(st, st_after, K, dtype, args.layout)
    no_tiles = (kern.startswith("k_sddmm_rb") and
                not st_after["rb_tiles"][{128: 0, 256: 1, 512: 2, 1024: 3, 2048: 4}[rby]])
    roof = {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "kernel": kern,
            "bytes_alg_per_launch": bytes_alg, "traffic_source": traffic_src}
    dtiles = st_after.get("dense_sampled_tiles", 0)
    if dtiles:  # sddmm.hip use_dense: whole 128 x 128 tiles on the matrix cores
        nw = 8 if dtiles < 512 else 4  # sddmm_dense.hip launch_dense (BSMR_DENSE_KS unset)
        kern = (f"k_sddmm_dense<{'f16' if dtype == 1 else 'bf16'},64,2,{nw}> (dense-sampled: "
                f"{dtiles} non-empty 128 x 128 MFMA tiles, {nw} waves per tile, K in 64-wide "
                "LDS-DMA chunks, stored entries sampled from the fp32 tile)")
        flops_tiles = 2.0 * dtiles * 128 * 128 * K
        ach = flops_tiles / (ms_per_step * 1e-3) / 1e12
        roof = {"bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_HALF_PEAK_TFS,
                "unit": "TFLOP/s", "frac": round(ach / MFMA_HALF_PEAK_TFS, 4), "traffic": traffic,
                "kernel": kern, "flops_alg_per_launch": flops_tiles,
                "traffic_source": traffic_src,
                "hbm_bytes_alg_per_launch": bytes_alg,
                "note": "algorithmic FLOPs of the tiles computed (the dense-sampled launch "
                        "computes every product of a non-empty tile)",
                # no credit for zero-padding - the sampled entries' own flops
                "achieved_sampled_flops": round(flops_rank / (ms_per_step * 1e-3) / 1e12, 3),
                "frac_sampled_flops": round(flops_rank / (ms_per_step * 1e-3) / 1e12 /
                                            MFMA_HALF_PEAK_TFS, 5),
                "frac_hbm": round(achieved / HBM_PEAK_GBS, 4)}
    out = {
        "metric": METRIC,
        "value": round(value, 2),
        "unit": "GFLOP/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 5),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": {0: "f32", 1: "f16", 2: "bf16"}[dtype],
        "data": "synthetic",
        "full": bool(args.full),
        "config": {
            "workload": desc + f", K={K}, BSMR alpha={args.alpha} delta={args.delta}",
            "M": M, "N": N, "nnz": nnz, "K": K, "alpha": args.alpha, "delta": args.delta,
            "parallelism": "single GPU, whole plan (one launch per step)",
            "num_clusters": st["num_clusters"], "dense_tiles": st["num_dense_tiles"],
            "residual_nnz": st["num_residual"],
            "plan_build_s": round(plan_s, 3), "row_reorder_ms": round(st["row_reorder_ms"], 3),
            "col_reorder_ms": round(st["col_reorder_ms"], 3),
            "rowblock_layout": {k: st_after[k] for k in ("rb_rows", "rb_items", "rb_pieces")},
            **({"tuning": args.tuning} if args.tuning else {}),
        },
        "roofline": roof,
        # the launch's dense-tile-only / residual-only halves (None when the layout keeps no
        # MFMA tiles: fp32 row-block plans demote every tile)
        "kernels_ms": {k: (None if k == "dense_ms" and no_tiles else round(v, 5))
                       for k, v in prof.items()},
    }
    if kern.startswith("k_sddmm_rb"):
        out["bounds"] = rowblock_bounds(st_after, rby, ms_per_step)
    mc = (traffic_src or {}).get("mfma_counters") if isinstance(traffic_src, dict) else None
    out["mfma"] = mfma_report(st, st_after, nnz, rby, dtiles, kern, no_tiles,
                              mfma_busy(mc, nnz, K) if mc else None)
    if (no_tiles and not dtiles and split and st["num_dense_tiles"] > 0
            and nnz <= 20_000_000):
        out["mfma"]["forced_tiles_split"] = forced_mfma_split(
            args, (M, N, rp, ci), K, dtype, dA, dB, dev, stream, P_gpu, flops_rank)
    out["timing"] = timing
    if cold_ms is not None:
        out["cold"] = {"ms_per_step": round(cold_ms, 5),
                       "value": round(flops_rank * world / (cold_ms * 1e-3) / 1e9, 2),
                       "note": "median of steps each preceded by a 512 MiB write (MALL evicted)"}
    if cold_clean_ms is not None:
        out["cold"]["clean"] = {
            "ms_per_step": round(cold_clean_ms, 5),
            "value": round(flops_rank * world / (cold_clean_ms * 1e-3) / 1e9, 2),
            "note": "median of steps each preceded by a 512 MiB read (MALL evicted, caches clean: "
                    "the launch writes back no dirty lines of the eviction)"}
    if args.full and not args.no_vendor:
        out["vendor_baseline"] = vendor_baseline(M, N, K, rp, ci, dA, dB, P_gpu, dtype, stream,
                                                 flops_rank, ms_per_step)
    if args.full and not args.no_cpu_baseline:
        if dtype == F32:
            Ar, Br = A, B
        else:  # the oracle runs in fp32 on the same rounded half values
            Ar = dA.float().cpu().numpy()
            Br = dB.float().cpu().numpy()
        out["cpu_baseline"] = cpu_baseline(M, N, rp, ci, K, Ar, Br, P_gpu)
    print(json.dumps(out), flush=True)


def sharded_workload(args, world):
    """(pattern, K, dtype, description, scaling) of a multi-GPU run: C2 weak (world stacked
    copies of the nips-like pattern), the other configs strong (one matrix split)."""
    from bsmr import synth

    (M, N, rp, ci), K, dtype, desc = workload(args)
    if args.config != "C2":
        return (M, N, rp, ci), K, dtype, desc, "strong"
    return (synth.stack_copies(M, N, rp, ci, world), K, dtype,
            desc + f"; x{world} stacked copies (copy b: columns relabelled by a random "
                   "permutation, synth.stack_copies), one C2 per GPU", "weak")


def _timed_steps(step, steps, warmup, stream, use_graph=True, has_work=True):
    """warmup untimed steps, then `steps` timed, bracketed by a barrier + device synchronisation
    on both sides; returns this rank's ms per step. step(h) issues one step on stream handle h
    (default: the launch stream). Timed as one HIP graph of the `steps` launches (graph_time)
    when use_graph and capture works on every rank, else (every rank) as stream launches between
    HIP events. has_work = False: this rank launches nothing (0 ms)."""
    import torch
    import torch.distributed as dist

    from bsmr import dist as D

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    if use_graph:
        dist.barrier()
        torch.cuda.synchronize()
        ms = graph_time(step, steps, stream.device)[0] if has_work else 0.0
        torch.cuda.synchronize()
        # the same method on every rank (the barriers below must pair up)
        if min(D.all_values(1.0 if ms is not None else 0.0, stream.device)) > 0:
            return ms
    dist.barrier()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        step()
    e1.record(stream)
    torch.cuda.synchronize()
    dist.barrier()
    return e0.elapsed_time(e1) / max(steps, 1)


def _host_ref(M, N, rp, ci, K, A, B, dtype, tdt):
    """The product's host SDDMM (host.cpp:45-76 restated) on the rounded inputs of the run."""
    import torch

    from bsmr import F32, sddmm_cpu

    if dtype == F32:
        Ar, Br = A, B
    else:
        Ar = torch.from_numpy(A).to(tdt).float().numpy()
        Br = torch.from_numpy(B).to(tdt).float().numpy()
    return sddmm_cpu(M, N, rp, ci, K, Ar, Br, threads=host_threads())


def _bcast_b(B_host, N, K, tdt, dev):
    """B generated on rank 0 and broadcast once over RCCL (xGMI); returns (dB, ms)."""
    import torch
    import torch.distributed as dist

    from bsmr import dist as D

    if dist.get_rank() == 0:
        dB = torch.from_numpy(B_host).to(dev).to(tdt)
    else:
        dB = torch.empty(N * K, dtype=tdt, device=dev)
    dist.barrier()
    torch.cuda.synchronize()
    tb = time.perf_counter()
    D.broadcast_(dB, 0)
    torch.cuda.synchronize()
    return dB, (time.perf_counter() - tb) * 1e3


def shard_global(args, rank, world, wl, dev, time_whole=False):
    """Row-panel shards of ONE global BSMR plan (the reference layout): rank 0
    clusters and broadcasts the row stage over RCCL, every rank rebuilds the column stage, cuts the
    same contiguous panel ranges, holds only its panels' A rows and runs bsmr_sddmm_panels_local;
    B broadcast once; P gathered to rank 0 compacted in plan order (bit-exact). time_whole: rank 0 also times the unsharded
    whole-plan launch (the N = 1 point of the same plan) before the shards run. Returns the
    report dict on rank 0 (with the gathered P under "_P"), None elsewhere."""
    import numpy as np
    import torch

    from bsmr import BsmrError, make_data
    from bsmr import dist as D

    (M, N, rp, ci), K, dtype, desc, scaling = wl
    nnz = len(ci)
    plan, pinfo = D.distribute_plan(M, N, rp, ci, dev, alpha=args.alpha, delta=args.delta,
                                    layout=args.layout)
    st = plan.stats()
    t0 = time.perf_counter()
    # the same cuts on every rank (same global plan): the model's, then re-balanced by measured
    # shard times (bsmr_plan_shard_rebalance) for args.rebalance rounds
    cuts = [plan.shard(K, r, world, dtype)[0] for r in range(world)] + [st["num_row_panels"]]
    cut_s = time.perf_counter() - t0
    rows = plan.array("reorderedRows")
    tdt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dtype]
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    # A partitioned: the makeData stream is a function of the row, so every rank derives its own
    # panels' rows locally (nothing of A is sent); only they reach this GPU
    A = make_data(M * K)
    B = make_data(N * K) if rank == 0 else None
    dB, bcast_ms = _bcast_b(B, N, K, tdt, dev)
    whole_ms = None
    if time_whole:  # rank 0: the same plan unsharded, whole A on this GPU
        if rank == 0:
            dA_all = torch.from_numpy(A).to(dev).to(tdt)
            dP1 = torch.zeros(nnz, dtype=torch.float32, device=dev)

            def whole(h=sp):
                plan.sddmm(dA_all.data_ptr(), dB.data_ptr(), K, dP1.data_ptr(), stream=h,
                           dtype=dtype)
        else:
            def whole(h=sp):
                pass
        whole_ms = _timed_steps(whole, args.steps, args.warmup, stream, not args.no_graph,
                                has_work=rank == 0)
        if rank == 0:
            del dA_all, dP1
            torch.cuda.empty_cache()
    dP = torch.zeros(nnz, dtype=torch.float32, device=dev)
    cur = {}

    def use(c):  # this rank's panels of cuts c and their A rows on the device
        cur["p0"], cur["p1"] = c[rank], c[rank + 1]
        A_local = D.shard_a_rows(A, K, rows, cur["p0"], cur["p1"])
        cur["dA"] = torch.from_numpy(A_local.reshape(-1)).to(dev).to(tdt)
        if cur["dA"].numel() == 0:
            cur["dA"] = torch.zeros(K, dtype=tdt, device=dev)

    def step(h=sp):
        if cur["p1"] > cur["p0"]:
            plan.sddmm_panels_local(cur["dA"].data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
                                    cur["p0"], cur["p1"], stream=h, dtype=dtype)

    rounds = []
    best = None
    for it in range(args.rebalance + 1):
        use(cuts)
        ms_r = D.all_values(_timed_steps(step, min(args.steps, 50), args.warmup, stream,
                                         not args.no_graph, cur["p1"] > cur["p0"]), dev)
        rounds.append({"cuts": [int(c) for c in cuts], "ms_per_step": [round(x, 5) for x in ms_r],
                       "imbalance_max_over_mean": round(max(ms_r) / (sum(ms_r) / world), 3)})
        if best is None or max(ms_r) < best[0]:
            best = (max(ms_r), list(cuts))
        if it == args.rebalance or world == 1:
            break
        try:
            nxt = plan.shard_rebalance(K, world, cuts, ms_r, dtype)
        except BsmrError:  # not a row-block launch: the per-panel model's cuts stay
            break
        if nxt == cuts:
            break
        cuts = nxt
    cuts = best[1]  # the fastest cut seen
    use(cuts)
    p0, p1 = cur["p0"], cur["p1"]
    ms_mine = _timed_steps(step, args.steps, args.warmup, stream, not args.no_graph,
                           cur["p1"] > cur["p0"])
    ms_all = D.all_values(ms_mine, dev)
    # every rank's output positions in plan order, from the plan every rank holds (nothing sent)
    pos_all = [D.shard_positions(rp, rows, cuts[r], cuts[r + 1]) for r in range(world)]
    counts = [len(x) for x in pos_all]
    mine = counts[rank]
    entries_all = [float(c) for c in counts]
    panels_all = D.all_values(p1 - p0, dev)
    torch.cuda.synchronize()
    tg = time.perf_counter()
    # each rank sends its outputs compacted in plan order, rank 0 scatters them (bit-exact)
    P = D.gather_compact(dP, pos_all[rank], counts, nnz, pos_all if rank == 0 else None, 0)
    gather_ms = (time.perf_counter() - tg) * 1e3
    st_after = plan.stats()
    if rank != 0:
        return None
    kern, _ = kernel_name(st, st_after, K, dtype, args.layout)
    ms = max(ms_all)
    out = {
        "split": "global",
        "parallelism": (f"row-panel shards x{world} of one global BSMR plan (rank 0 clusters, row "
                        "stage broadcast over RCCL, column stage rebuilt per rank), A rows local "
                        "to their shard, B broadcast once (RCCL), P gathered to rank 0 compacted "
                        "in plan order (bit-exact)"),
        "ms_per_step": round(ms, 5),
        "value": round(2.0 * nnz * K / (ms * 1e-3) / 1e9, 2),
        "num_clusters": st["num_clusters"], "num_row_panels": st["num_row_panels"],
        "plan_build_s": round(pinfo["plan_build_s"], 3),
        "row_reorder_ms": round(st["row_reorder_ms"], 3),
        "plan_distribution_ms": round(pinfo["distribute_ms"], 3),
        "row_stage_bcast_ms": round(pinfo["row_stage_bcast_ms"], 3),
        "row_stage_bytes": pinfo["row_stage_bytes"],
        "shard_cut_s": round(cut_s, 3),
        "rebalance_rounds": rounds,
        "b_broadcast_ms": round(bcast_ms, 3),
        "p_gather_ms": round(gather_ms, 3),
        "shards": {
            "panels": [int(x) for x in panels_all],
            "entries": [int(x) for x in entries_all],
            "ms_per_step": [round(x, 5) for x in ms_all],
            "imbalance_max_over_mean": round(ms / (sum(ms_all) / world), 3),
            "kernel": "bsmr_sddmm_panels_local -> " + kern,
        },
        "_P": P,
    }
    if whole_ms is not None:
        out["whole_plan_one_gpu"] = {
            "ms_per_step": round(whole_ms, 5),
            "value": round(2.0 * nnz * K / (whole_ms * 1e-3) / 1e9, 2),
            "note": "rank 0 alone, the same global plan unsharded (bsmr_sddmm), timed in this run",
            "speedup_of_split": round(whole_ms / ms, 3),
            "strong_scaling_efficiency": round(whole_ms / ms / world, 3)}
    return out


def shard_local(args, rank, world, wl, dev):
    """S cut into `world` contiguous original row panels of equal stored entries; rank r clusters
    and lays out its own panel (a local BSMR plan over rows [r0, r1)), stages only those A rows,
    receives B once over RCCL and writes P[rowptr[r0]:rowptr[r1]] (contiguous CSR positions),
    gathered to rank 0 segment by segment. No plan crosses ranks. Returns the report dict on
    rank 0 (gathered P under "_P"), None elsewhere.
    One-GPU rehearsal (tools/shard_sim.py, each shard timed alone): reddit-like x1, 8 shards:
    slowest 0.600 ms, imbalance 1.02 (global-plan shards: 0.726 ms, 1.19); C2 weak-scaling
    copies at N = 2 / 4 / 8: 11.5 / 11.4 / 11.8 us (global 11.7 / 13.4 / 13.5 us), one C2 11.2 us
    (profiles/r02c/c4_shards/, profiles/r02c/weak_scaling/)."""
    import numpy as np
    import torch

    from bsmr import Plan, make_data, sddmm_cpu
    from bsmr import dist as D

    (M, N, rp, ci), K, dtype, desc, scaling = wl
    nnz = len(ci)
    rp64 = np.asarray(rp, dtype=np.int64)
    r0, r1 = D.row_range_cut(rp64, rank, world)
    e0, e1 = int(rp64[r0]), int(rp64[r1])
    rp_loc = (rp64[r0:r1 + 1] - e0).astype(np.uint32)
    ci_loc = np.ascontiguousarray(np.asarray(ci)[e0:e1], dtype=np.uint32)
    t0 = time.perf_counter()
    # bsmr_plan_create needs >= 2 stored entries: a panel with fewer (only when nnz < 2 world)
    # has no launch; its one entry, if any, is computed by the product's host SDDMM below
    plan = (Plan(r1 - r0, N, rp_loc, ci_loc, alpha=args.alpha, delta=args.delta,
                 layout=args.layout) if e1 - e0 >= 2 else None)
    plan_s = time.perf_counter() - t0
    st = plan.stats() if plan else None
    tdt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dtype]
    # A partitioned: the makeData stream is a function of the row, so every rank derives its own
    # rows locally (nothing of A is sent)
    A = make_data(M * K)
    B = make_data(N * K) if rank == 0 else None
    dA = torch.from_numpy(np.ascontiguousarray(A[r0 * K:max(r1, r0 + 1) * K])).to(dev).to(tdt)
    dB, bcast_ms = _bcast_b(B, N, K, tdt, dev)
    dP_loc = torch.zeros(max(e1 - e0, 1), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream

    def step(h=sp):
        if plan:
            plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP_loc.data_ptr(), stream=h, dtype=dtype)

    ms_mine = _timed_steps(step, args.steps, args.warmup, stream, not args.no_graph,
                           plan is not None)
    if plan is None and e1 - e0 == 1:
        Ah = dA.float().cpu().numpy().reshape(-1)
        Bh = dB.float().cpu().numpy()
        dP_loc[0] = float(sddmm_cpu(r1 - r0, N, rp_loc, ci_loc, K, Ah, Bh)[0])
    ms_all = D.all_values(ms_mine, dev)
    entries_all = D.all_values(e1 - e0, dev)
    rows_all = D.all_values(r1 - r0, dev)
    plan_all = D.all_values(plan_s, dev)
    torch.cuda.synchronize()
    tg = time.perf_counter()
    P = D.gather_segments(dP_loc, e0, e1, nnz, 0)
    gather_ms = (time.perf_counter() - tg) * 1e3
    st_after = plan.stats() if plan else None
    if rank != 0:
        return None
    kern = kernel_name(st, st_after, K, dtype, args.layout)[0] if st else "none (empty panel)"
    ms = max(ms_all)
    return {
        "split": "local",
        "parallelism": (f"row-panel shards x{world} of S in original row order (contiguous "
                        "panels of equal stored entries), each rank's BSMR plan built on its own "
                        "panel, A rows local, B broadcast once (RCCL), P segments gathered to "
                        "rank 0"),
        "ms_per_step": round(ms, 5),
        "value": round(2.0 * nnz * K / (ms * 1e-3) / 1e9, 2),
        "plan_build_s_max": round(max(plan_all), 3),
        "b_broadcast_ms": round(bcast_ms, 3),
        "p_gather_ms": round(gather_ms, 3),
        "shards": {
            "rows": [int(x) for x in rows_all],
            "entries": [int(x) for x in entries_all],
            "ms_per_step": [round(x, 5) for x in ms_all],
            "imbalance_max_over_mean": round(ms / (sum(ms_all) / world), 3),
            "kernel": "bsmr_sddmm (rank-local plan) -> " + kern,
        },
        "_P": P,
    }


def strong_c4(args, rank, world, dev):
    """The north_star multi-GPU config (BASELINE.json C4): reddit-like Chung-Lu graph at
    --strong-scale (232 M stored entries at 1), fp32 K = 128, row-panel sharded over the run's
    ranks in both splits: the global plan (reference layout; rank 0 also times
    the unsharded plan = the N = 1 point) and the local one. The pattern is generated on rank 0 and
    broadcast over RCCL. Both gathered P are checked against the product host SDDMM."""
    import numpy as np
    import torch
    import torch.distributed as dist

    from bsmr import F32, check_data, make_data, synth
    from bsmr import dist as D

    t0 = time.perf_counter()
    n = max(1024, int(232965 * args.strong_scale))
    if rank == 0:
        M, N, rp, ci = synth.reddit_like(args.strong_scale)
        lens = torch.tensor([M, len(ci)], dtype=torch.int64, device=dev)
    else:
        lens = torch.zeros(2, dtype=torch.int64, device=dev)
    D.broadcast_(lens, 0)
    M, nnz = int(lens[0]), int(lens[1])
    assert M == n
    d_rp = (torch.from_numpy(rp.view(np.int32)).to(dev) if rank == 0
            else torch.empty(M + 1, dtype=torch.int32, device=dev))
    d_ci = (torch.from_numpy(ci.view(np.int32)).to(dev) if rank == 0
            else torch.empty(nnz, dtype=torch.int32, device=dev))
    D.broadcast_(d_rp, 0)
    D.broadcast_(d_ci, 0)
    rp = d_rp.cpu().numpy().view(np.uint32)
    ci = d_ci.cpu().numpy().view(np.uint32)
    del d_rp, d_ci
    gen_s = time.perf_counter() - t0
    K, dtype = 128, F32
    desc = (f"C4: reddit_like Chung-Lu power law x{args.strong_scale} (seed 20250803), "
            f"{M}^2, {nnz:,} stored entries, fp32 A/B, K={K}")
    wl = ((M, M, rp, ci), K, dtype, desc, "strong")
    res = {}
    for split in ("global", "local"):
        try:
            if split == "global":
                r = shard_global(args, rank, world, wl, dev, time_whole=True)
            else:
                r = shard_local(args, rank, world, wl, dev)
        except Exception as e:  # noqa: BLE001 - reported in the line; the C2 value still prints
            r = {"error": f"{type(e).__name__}: {e}"[:400]} if rank == 0 else None
        torch.cuda.empty_cache()
        res[split] = r
        dist.barrier()
    if rank != 0:
        return None
    ref = _host_ref(M, M, rp, ci, K, make_data(M * K), make_data(M * K), dtype, torch.float32)
    for split in ("global", "local"):
        r = res[split]
        if r is not None and "_P" in r:
            r["checkData_errors_gathered_P"] = check_data(ref, r.pop("_P"))
    flops = 2.0 * nnz * K
    return {"workload": desc, "M": M, "nnz": nnz, "K": K, "n_gpus": world,
            "flops_per_step": flops, "pattern_gen_and_bcast_s": round(gen_s, 2),
            "global": res["global"], "local": res["local"],
            "note": "strong scaling of the one matrix; value = 2 nnz K / slowest rank's ms; "
                    "whole_plan_one_gpu (global) is the N = 1 point measured in the same run"}


def main_sharded(args, rank, world):
    """Multi-GPU line: the config's row-panel split (--shard; C2 = weak scaling over stacked
    copies, the line's `value`), plus for C2 at N > 1 (or --strong on) the north_star reddit
    split (strong_C4 block: both splits, the N = 1 point of the global plan, per-rank ms,
    imbalance, broadcast and plan times)."""
    import torch
    import torch.distributed as dist

    from bsmr import check_data

    dev = torch.device("cuda", torch.cuda.current_device())
    wl = sharded_workload(args, world)
    (M, N, rp, ci), K, dtype, desc, scaling = wl
    mode = "global" if args.shard == "global" else "local"
    r = (shard_global(args, rank, world, wl, dev) if mode == "global"
         else shard_local(args, rank, world, wl, dev))
    do_strong = args.strong == "on" or (args.strong == "auto" and args.full and world > 1
                                        and args.config == "C2")
    strong = strong_c4(args, rank, world, dev) if do_strong else None
    if rank != 0:
        dist.destroy_process_group()
        return
    tdt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dtype]
    from bsmr import make_data
    P = r.pop("_P")
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, P)
    nerr = None
    if args.full:  # the gathered P against the product's host SDDMM
        ref = _host_ref(M, N, rp, ci, K, make_data(M * K), make_data(N * K), dtype, tdt)
        nerr = check_data(ref, P)
    nnz = len(ci)
    ms = r["ms_per_step"]
    s = 4 if dtype == 0 else 2
    bytes_alg = s * K * (M + N) + 4.0 * nnz + 4.0 * (M + 1) + 4.0 * nnz
    achieved = bytes_alg / (ms * 1e-3) / 1e9
    cfg = {"workload": desc + f", K={K}, BSMR alpha={args.alpha} delta={args.delta}",
           "M": M, "N": N, "nnz": nnz, "K": K, "alpha": args.alpha, "delta": args.delta,
           "parallelism": r.pop("parallelism"), "shard_mode": mode, "backend": dist.get_backend()}
    if args.tuning:
        cfg["tuning"] = args.tuning
    for k in list(r):
        if k not in ("split", "ms_per_step", "value", "shards"):
            cfg[k] = r.pop(k)
    out = {
        "metric": METRIC,
        "value": r["value"],
        "unit": "GFLOP/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms,
        "higher_is_better": True,
        "scaling": scaling,
        "vs_baseline": None,
        "dtype": {0: "f32", 1: "f16", 2: "bf16"}[dtype],
        "data": "synthetic",
        "full": bool(args.full),
        "config": cfg,
        "shards": r["shards"],
        "roofline": {"bound": "hbm", "achieved": round(achieved, 2),
                     "peak": HBM_PEAK_GBS * world, "unit": "GB/s",
                     "frac": round(achieved / (HBM_PEAK_GBS * world), 4), "traffic": None,
                     "kernel": r["shards"]["kernel"], "bytes_alg_per_launch": bytes_alg,
                     "note": "whole-job algorithmic bytes per step over the slowest rank's time, "
                             "against world x 8 TB/s"},
        "checkData_errors_gathered_P": nerr,
    }
    if scaling == "weak":
        out["scaling_detail"] = (
            "independent replicas: the global pattern is N stacked copies of C2 (columns "
            "relabelled per copy) and each rank plans and runs its own copy, so per-GPU work is "
            "one C2 and nothing crosses ranks in the timed loop; the north_star row-panel split "
            "of one matrix is the strong_C4 block (global plan clustered once, its N = 1 point "
            "measured in the same run)")
    if strong is not None:
        out["strong_C4"] = strong
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    rc = main()
    sys.exit(rc if isinstance(rc, int) else 0)
