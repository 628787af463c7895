"""Helpers for the GPU tests: device buffers through torch (plumbing only), oracle comparisons."""
import numpy as np

import oracle_lib as O


def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return torch


def run_sddmm(plan, A, B, K, nnz, panels=None, dtype=0):
    """P (fp32, NaN where not written) of the whole plan or of the given panel ranges; dtype 1/2
    rounds A and B to fp16/bf16 on the device (compare against the oracle on half_values())."""
    torch = torch_cuda()
    tdt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dtype]
    dA = torch.from_numpy(np.ascontiguousarray(A, np.float32)).cuda().to(tdt)
    dB = torch.from_numpy(np.ascontiguousarray(B, np.float32)).cuda().to(tdt)
    dP = torch.full((max(nnz, 1),), float("nan"), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if panels is None:
        plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), stream=s, dtype=dtype)
    else:
        for p0, p1 in panels:
            plan.sddmm_panels(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), p0, p1, stream=s,
                              dtype=dtype)
    torch.cuda.synchronize()
    return dP.cpu().numpy()[:nnz]


def oracle_plan(M, N, rowptr, colidx, alpha, delta, free_mem):
    c = O.CSR.from_arrays(M, N, rowptr, colidx)
    bs = O.block_size(M, N, free_mem)
    rows, ncl, _ = O.row_reorder(c, np.float32(alpha), bs)
    return c, O.Plan(c, rows, ncl, np.float32(delta)), ncl


PLAN_ARRAYS = ["reorderedRows", "denseCols", "denseColOffsets", "sparseCols", "sparseColOffsets",
               "sparseValueOffsets", "blockOffsets", "blockValues", "sparseValues",
               "sparseRelativeRows", "sparseColIndices"]


def assert_plans_equal(gpu_plan, orc_plan):
    for name in PLAN_ARRAYS:
        g = gpu_plan.array(name)
        o = orc_plan.array(name)
        assert g.shape == o.shape, (name, g.shape, o.shape)
        if not np.array_equal(g, o):
            bad = np.nonzero(g != o)[0]
            raise AssertionError(f"{name}: {len(bad)} mismatches, first at {bad[:5]}: "
                                 f"gpu {g[bad[:5]]} oracle {o[bad[:5]]}")


def half_values(X, dtype):
    """X rounded (RNE) to fp16 (dtype 1) or bf16 (2), back in fp32: the values the kernel sees.
    Host only (the device does the same rounding in run_sddmm)."""
    import torch
    tdt = {1: torch.float16, 2: torch.bfloat16}[dtype]
    return torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(tdt).float().numpy()


def torch_dtype(dtype):
    torch = torch_cuda()
    return {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dtype]


def to_device(X, dtype):
    """X (fp32 on the host) as a device tensor of `dtype`, converted on the host so that the device
    holds exactly the bits of half_values(X, dtype)."""
    torch = torch_cuda()
    return torch.from_numpy(np.array(X, np.float32)).to(torch_dtype(dtype)).cuda()


def nan_output(n):
    torch = torch_cuda()
    return torch.full((max(int(n), 1),), float("nan"), dtype=torch.float32, device="cuda")


def sddmm_once(plan, A, B, K, nnz, dtype=0):
    """P (numpy fp32, nnz) of one bsmr_sddmm on host operands; P starts as NaN."""
    torch = torch_cuda()
    dA, dB, dP = to_device(A, dtype), to_device(B, dtype), nan_output(nnz)
    plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
               stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    return dP.cpu().numpy()[:nnz]


def spmm_launch(plan, side, dV, dX, K, dtype, dY, stream=None):
    """One bsmr_spmm (side 1) / bsmr_spmm_t (side 2) on device tensors, on `stream` (a torch
    stream) or the current one; no synchronisation."""
    torch = torch_cuda()
    s = (stream or torch.cuda.current_stream()).cuda_stream
    fn = plan.spmm if side == 1 else plan.spmm_t
    fn(dV.data_ptr(), dX.data_ptr(), K, dY.data_ptr(), stream=s, dtype=dtype)


def spmm_device(plan, side, dV, dX, K, dtype):
    """Y (numpy fp32, destinations x K) of one launch on device operands; Y starts as NaN."""
    torch = torch_cuda()
    rows = plan.M if side == 1 else plan.N
    dY = torch.full((rows, K), float("nan"), dtype=torch.float32, device="cuda")
    spmm_launch(plan, side, dV, dX, K, dtype, dY)
    torch.cuda.synchronize()
    return dY.cpu().numpy()


def spmm_once(plan, side, V, X, K, dtype=0):
    """Y (numpy fp32) of one launch on host operands: V (fp32, nnz) and X (fp32 on the host,
    converted there so that the device holds exactly the bits of half_values(X, dtype))."""
    torch = torch_cuda()
    dV = torch.from_numpy(np.ascontiguousarray(V, np.float32)).cuda()
    return spmm_device(plan, side, dV, to_device(X, dtype), K, dtype)


def rb_geometry(plan, K, dtype):
    """The whole-plan row-block layout of (K, dtype) through the library's debug export (not in the
    header): rows per block, threads per workgroup, item slots, row bytes; None when that (K, dtype)
    does not run the row-block launch. Builds the layout if no launch has."""
    import ctypes as C

    import bsmr
    L = bsmr.lib()
    L.bsmr_debug_rb_items.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    n = C.c_uint64()
    assert L.bsmr_debug_rb_items(plan.h, K, dtype, None, C.byref(n)) == 0
    if n.value == 0:
        return None
    buf = np.zeros(n.value, np.uint32)
    assert L.bsmr_debug_rb_items(plan.h, K, dtype, buf.ctypes.data, C.byref(n)) == 0
    return dict(rb=int(buf[0]), nt=int(buf[1]), items=int(buf[2]), row_bytes=int(buf[3]))


STORE_HEAD = ("outLds", "outCap", "outRuns", "outPacked", "NT", "nItems", "prpw", "xcds")


def rb_store(plan, K, dtype, raw=True, panels=None):
    """How the whole-plan row-block layout of (K, dtype) writes P, through the library's debug
    exports bsmr_debug_rb_store and bsmr_debug_rb_pieces (not in the header); None when that
    (K, dtype) does not run the row-block launch. The dict store_cases.classify reads: the header
    (STORE_HEAD; prpw = PAIR_RUNS_PER_WAVE, xcds = XCD_BUCKETS, the library's constants), per item
    slot in launch order ent (entries), nruns, longest, shortest (0 without a run table), rb (row
    block), real (not padding), and with raw the tables of a staged layout: itemEnt (n x 2) and
    itemRuns (n x 2) + runs (r x 2), or sortedPos. Builds the layout if no launch has.
    panels = (p0, p1): the same of the layout bsmr_sddmm_panels runs over that range
    (bsmr_debug_rb_store_panels), with the form of its launch: pairs, dyn, lite (booleans), grid."""
    import ctypes as C

    import bsmr
    L = bsmr.lib()
    args = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    L.bsmr_debug_rb_store.argtypes = args
    L.bsmr_debug_rb_pieces.argtypes = args
    L.bsmr_debug_rb_store_panels.argtypes = args[:3] + [C.c_uint32, C.c_uint32] + args[3:]
    if panels is None:
        export = lambda out, n: L.bsmr_debug_rb_store(plan.h, K, dtype, out, n)  # noqa: E731
        nh, per = 8, 4
    else:
        export = lambda out, n: L.bsmr_debug_rb_store_panels(plan.h, K, dtype, panels[0], panels[1], out, n)  # noqa: E731
        nh, per = 12, 6
    n = C.c_uint64(0)
    assert export(None, C.byref(n)) == 0, L.bsmr_last_error()
    if n.value == 0:
        return None
    buf = np.zeros(n.value, np.uint32)  # (the whole export: a buffer of the item words alone gets no raw tables)
    want = C.c_uint64(n.value)
    assert export(buf.ctypes.data, C.byref(want)) == 0
    assert want.value == n.value
    d = dict(zip(STORE_HEAD, (int(x) for x in buf[:8])))
    d["outRuns"], d["outPacked"] = bool(d["outRuns"]), bool(d["outPacked"])
    ni = d["nItems"]
    item = buf[nh:nh + per * ni].reshape(-1, per)
    d.update(ent=item[:, 0].copy(), nruns=item[:, 1].copy(), longest=item[:, 2].copy(), shortest=item[:, 3].copy(),
             itemEnt=None, itemRuns=None, runs=None, sortedPos=None)
    if d["outLds"] and raw:
        o = nh + per * ni
        d["itemEnt"] = buf[o:o + 2 * ni].reshape(-1, 2).copy()
        o += 2 * ni
        if d["outRuns"]:
            d["itemRuns"] = buf[o:o + 2 * ni].reshape(-1, 2).copy()
            d["runs"] = buf[o + 2 * ni:].reshape(-1, 2).copy()
            assert len(d["runs"]) == int(d["nruns"].sum())
        else:
            d["sortedPos"] = buf[o:].copy()
            assert len(d["sortedPos"]) == int(d["ent"].sum())
    if panels is not None:
        d.update(pairs=bool(buf[8]), dyn=bool(buf[9]), lite=bool(buf[10]), grid=int(buf[11]),
                 rb=item[:, 4].copy(), real=item[:, 5].astype(bool))
        return d
    assert L.bsmr_debug_rb_pieces(plan.h, K, dtype, None, C.byref(n)) == 0
    pb = np.zeros(n.value, np.uint32)
    assert L.bsmr_debug_rb_pieces(plan.h, K, dtype, pb.ctypes.data, C.byref(n)) == 0
    assert int(pb[0]) == ni
    items = pb[2:2 + 4 * ni].reshape(-1, 4)
    ends = pb[2 + 4 * ni:2 + 5 * ni]
    d["rb"] = items[:, 0].copy()
    d["real"] = ~((items[:, 1] == items[:, 2]) & (items[:, 3] == ends))  # (k_sddmm_rb's padding test)
    return d


def store_constants():
    """{prpw, xcds, run_max}: PAIR_RUNS_PER_WAVE, XCD_BUCKETS and RB_RUN_MAX from the library
    (bsmr_debug_rb_store_constants; needs no device)."""
    import bsmr
    f = bsmr.lib().bsmr_debug_rb_store_constants
    f.argtypes = [np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")]
    out = np.zeros(3, np.uint32)
    assert f(out) == 0
    return dict(prpw=int(out[0]), xcds=int(out[1]), run_max=int(out[2]))


LAUNCH_KINDS = ("ptile", "dense", "rowblock", "half", "colmajor")  # csrc/launch_select.hpp Launch
RB_FORM = ("stageNt", "lateB", "pairs", "lite", "dyn", "NT", "grid", "ldsBytes", "stageBlocks")


def plan_launch(plan, K, dtype):
    """What bsmr_sddmm runs on `plan` for (K, dtype), as the library decides it (the debug export
    bsmr_debug_plan_launch, not in the header): dict(kind=a sddmm_cases kind, slot=the row-block
    slot or -1, row_bytes) and, for the row-block kind, the kernel form of the whole launch: lite,
    pairs, dyn (booleans), NT, grid, ... (RB_FORM) and packed (the layout keeps the CSR position in
    its metadata words and no `out` array). Builds the row-block layout if no launch has."""
    import ctypes as C

    import bsmr
    f = bsmr.lib().bsmr_debug_plan_launch
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_int, np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")]
    out = np.zeros(13, np.uint32)
    assert f(plan.h, K, dtype, out) == 0, bsmr.lib().bsmr_last_error()
    w = [int(x) for x in out]
    d = dict(kind=LAUNCH_KINDS[w[0]], slot=w[1] - 1, row_bytes=w[2])
    if d["kind"] == "rowblock":
        d.update(zip(RB_FORM, w[3:12]))
        for k in RB_FORM[:5]:
            d[k] = bool(d[k])
        d["packed"] = bool(w[12])
    return d


def path_evidence(case, plan):
    """Failures (strings) of a sddmm_cases.Case's evidence that its launch path ran, after the
    launch: sddmm_cases.check_stats on the plan's stats, the library's own account of the launch
    (plan_launch) and, for the row-block launch, its layout geometry, for the panel-tile launch the
    plan's tile offsets and the device's CU count."""
    from sddmm_cases import check_stats
    launch = plan_launch(plan, case.K, case.dtype)
    geom = store = None
    if case.kind == "rowblock":
        geom = rb_geometry(plan, case.K, case.dtype)
        store = rb_store(plan, case.K, case.dtype, raw=False)
    elif case.kind == "ptile":
        cus = torch_cuda().cuda.get_device_properties(0).multi_processor_count
        geom = dict(block_offsets=plan.array("blockOffsets"), cus=int(cus))
    bad = check_stats(case, plan.stats(), launch, geom, store)
    shown = dict(geom, block_offsets="...") if geom and "block_offsets" in geom else geom
    return [f"{b} (launch {launch}, geometry {shown}, stats {plan.stats()})" for b in bad]
