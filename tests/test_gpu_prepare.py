"""GPU: the explicit layout build (bsmr_plan_prepare / Plan.prepare) and HIP-graph capture of a
plan's first SDDMM.

The reference builds and uploads every RPHM array in its constructor, before sddmm_gpu
(src/BSMR.cpp:83-265); here the launch layout of a (K, dtype) is built on first use unless
Plan.prepare built it. These tests never warm a plan up: each builds a fresh Plan, prepares it (or
not) and captures its very first launch with torch.cuda.graph on a side stream.

* after prepare, the first sddmm / sddmm_batch / sddmm_panels / sddmm_panels_local of every launch
  kind (row-block fp32 and fp16, original-order rows, panel-tile, dense-sampled, column-major)
  captures into a graph whose replay matches the oracle's host SDDMM, reads the caller's buffers
  (A overwritten between replays) and writes every output (P starts as NaN);
* without prepare, the launch under capture raises BsmrError with status NOT_PREPARED, the capture
  survives (its other node, a memset of P, replays), and the same call outside capture builds
  lazily as it always did;
* prepared panel ranges survive any number of lazy range builds;
* recolumn drops what depends on the column split, the panel-tile item list included.

Values: oracle_lib.sddmm_cpu on the fp16/bf16-rounded operands (a product of two halves is exact
in fp32, so checkData's rule applies unchanged), as tests/test_gpu_ptile.py.
"""
import numpy as np
import pytest

import oracle_lib as O
import bsmr
from bsmr import BF16, F16, F32, Plan, make_data, synth
from gpu_util import half_values, torch_cuda

pytestmark = pytest.mark.gpu

FREE = 288 * 1024 ** 3

ZIPF = lambda: synth.random_rows(517, 4000, 60, seed=2, zipf=1.1)  # noqa: E731

# name: (pattern, K, dtype, plan kwargs, what the stats show once the named layout is built)
CASES = {
    "rb_f32": (ZIPF, 64, F32, {}, lambda st: st["rb_items"][1] > 0),
    "rb_f16": (ZIPF, 128, F16, {}, lambda st: st["rb_items"][1] > 0),
    "orig_rows": (lambda: synth.trefethen(3000), 64, F32, {"tuning": {"orig_rows": 1}},
                  lambda st: st["rb_orig_rows"] != 0),
    "ptile": (lambda: synth.block_mask(512, 16, 0.15, seed=11), 128, BF16, {},
              lambda st: st["ptile_items"] > 0),
    "dense": (lambda: synth.uniform_mask(512, 0.1, 7), 512, BF16, {},
              lambda st: st["dense_sampled_tiles"] > 0),
    "colmajor": (ZIPF, 16, F32, {}, None),
}


def _tdt(torch, dtype):
    return {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}[dtype]


def _ref(M, N, rp, ci, K, A, B, dtype):
    if dtype != F32:
        A, B = half_values(A, dtype), half_values(B, dtype)
    return O.sddmm_cpu(O.CSR.from_arrays(M, N, rp, ci), K, A, B)


def _dev(torch, X, dtype):
    return torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda().to(_tdt(torch, dtype))


def _nan(torch, n):
    return torch.full((max(n, 1),), float("nan"), dtype=torch.float32, device="cuda")


def _capture(torch, fn):
    """fn(stream) recorded into a graph on a side stream (a plain chain of nodes)."""
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(side.cuda_stream)
    return g


def _replay(torch, g, dP, nnz):
    g.replay()
    torch.cuda.synchronize()
    return dP.cpu().numpy()[:nnz]


def _assert_matches(ref, P):
    assert np.isfinite(P).all(), f"{int((~np.isfinite(P)).sum())} outputs never written"
    assert O.check_data(ref, P) == 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_first_sddmm_captured_after_prepare(case):
    torch = torch_cuda()
    pat, K, dtype, kw, built = CASES[case]
    M, N, rp, ci = pat()
    nnz = len(ci)
    plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, **kw)
    if built is None:  # the column-major launch has no lazy layout
        assert plan.prepared(K, dtype)
    else:
        assert not plan.prepared(K, dtype)
    plan.prepare(K, dtype)
    assert plan.prepared(K, dtype)
    if built is not None:
        assert built(plan.stats()), plan.stats()  # the case runs the launch it names
    A = make_data(M * K)
    B = make_data(N * K)
    A2 = (2.0 - A[::-1]).astype(np.float32)
    dA, dB, dP = _dev(torch, A, dtype), _dev(torch, B, dtype), _nan(torch, nnz)
    torch.cuda.synchronize()
    g = _capture(torch, lambda s: plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
                                             stream=s, dtype=dtype))
    _assert_matches(_ref(M, N, rp, ci, K, A, B, dtype), _replay(torch, g, dP, nnz))
    # the graph reads the caller's buffers, not a captured copy
    dA.copy_(_dev(torch, A2, dtype))
    dP.fill_(float("nan"))
    _assert_matches(_ref(M, N, rp, ci, K, A2, B, dtype), _replay(torch, g, dP, nnz))


@pytest.mark.parametrize("case", ["rb_f32", "ptile", "dense"])
def test_unprepared_capture_reports_not_prepared(case):
    torch = torch_cuda()
    pat, K, dtype, kw, _ = CASES[case]
    M, N, rp, ci = pat()
    nnz = len(ci)
    plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, **kw)
    A = make_data(M * K)
    B = make_data(N * K)
    dA, dB, dP = _dev(torch, A, dtype), _dev(torch, B, dtype), _nan(torch, nnz)
    torch.cuda.synchronize()
    caught = []

    def body(s):
        dP.zero_()
        with pytest.raises(bsmr.BsmrError) as ei:
            plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), stream=s, dtype=dtype)
        caught.append(ei.value)

    g = _capture(torch, body)  # ends normally: the refused launch did not invalidate the capture
    assert caught[0].status == bsmr.NOT_PREPARED
    assert "bsmr_sddmm: stream is capturing" in str(caught[0])
    assert "bsmr_plan_prepare first" in str(caught[0])
    P = _replay(torch, g, dP, nnz)
    assert (P == 0).all()
    assert not plan.prepared(K, dtype)
    # outside capture the same call builds lazily, as before
    dP.fill_(float("nan"))
    plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
               stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    _assert_matches(_ref(M, N, rp, ci, K, A, B, dtype), dP.cpu().numpy()[:nnz])
    assert plan.prepared(K, dtype)


def test_profile_refuses_a_capturing_stream():
    """bsmr_sddmm_profile synchronises events by design: BSMR_ERR_UNSUPPORTED (6) under capture,
    prepared or not, and the capture goes on."""
    torch = torch_cuda()
    pat, K, dtype, kw, _ = CASES["rb_f32"]
    M, N, rp, ci = pat()
    nnz = len(ci)
    plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, **kw)
    plan.prepare(K, dtype)
    dA, dB, dP = _dev(torch, make_data(M * K), dtype), _dev(torch, make_data(N * K), dtype), _nan(torch, nnz)
    torch.cuda.synchronize()
    caught = []

    def body(s):
        dP.zero_()
        with pytest.raises(bsmr.BsmrError) as ei:
            plan.profile(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), iters=1, stream=s)
        caught.append(ei.value)

    g = _capture(torch, body)
    assert caught[0].status == 6 and "bsmr_sddmm_profile: stream is capturing" in str(caught[0])
    assert (_replay(torch, g, dP, nnz) == 0).all()
    t = plan.profile(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), iters=1,
                     stream=torch.cuda.current_stream().cuda_stream)
    assert t["total_ms"] > 0


def test_panel_shards_captured():
    torch = torch_cuda()
    pat, K, dtype, kw, _ = CASES["rb_f32"]
    M, N, rp, ci = pat()
    nnz = len(ci)
    A = make_data(M * K)
    B = make_data(N * K)
    ref = _ref(M, N, rp, ci, K, A, B, dtype)
    dA, dB = _dev(torch, A, dtype), _dev(torch, B, dtype)
    for local in (False, True):
        plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, **kw)
        shards = [plan.shard(K, r, 2) for r in range(2)]
        assert shards[0][0] == 0 and shards[0][1] == shards[1][0] and shards[0][1] < shards[1][1]
        rows = plan.array("reorderedRows")
        if local:
            dAs = [_dev(torch, A.reshape(M, K)[rows[16 * p0:16 * p1]].reshape(-1), dtype)
                   for p0, p1 in shards]
            launch = plan.sddmm_panels_local
        else:
            dAs = [dA, dA]
            launch = plan.sddmm_panels
        dP = _nan(torch, nnz)
        torch.cuda.synchronize()
        for p0, p1 in shards:
            assert not plan.prepared(K, panels=(p0, p1), local=local)
        if local:  # an unprepared local shard launch is refused under capture
            caught = []

            def refused(s):
                dP.zero_()
                with pytest.raises(bsmr.BsmrError) as ei:
                    launch(dAs[0].data_ptr(), dB.data_ptr(), K, dP.data_ptr(), *shards[0], stream=s)
                caught.append(ei.value)

            _capture(torch, refused)
            assert caught[0].status == bsmr.NOT_PREPARED
            assert "bsmr_sddmm_panels_local: stream is capturing" in str(caught[0])
            assert "bsmr_plan_prepare_panels first" in str(caught[0])
            dP.fill_(float("nan"))
            torch.cuda.synchronize()
        for p0, p1 in shards:
            plan.prepare(K, panels=(p0, p1), local=local)
            assert plan.prepared(K, panels=(p0, p1), local=local)

        def both(s):
            for dAi, (p0, p1) in zip(dAs, shards):
                launch(dAi.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), p0, p1, stream=s)

        g = _capture(torch, both)
        _assert_matches(ref, _replay(torch, g, dP, nnz))


def test_batch_captured():
    torch = torch_cuda()
    pat, K, dtype, kw, built = CASES["ptile"]
    M, N, rp, ci = pat()
    nb, nnz = 3, len(ci)
    plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, **kw)
    A = make_data(nb * M * K)
    B = make_data(nb * N * K)[::-1].copy()
    dA, dB, dP = _dev(torch, A, dtype), _dev(torch, B, dtype), _nan(torch, nb * nnz)
    plan.prepare(K, dtype)
    assert plan.prepared(K, dtype) and built(plan.stats())
    torch.cuda.synchronize()
    g = _capture(torch, lambda s: plan.sddmm_batch(nb, dA.data_ptr(), dB.data_ptr(), K,
                                                   dP.data_ptr(), stream=s, dtype=dtype))
    P = _replay(torch, g, dP, nb * nnz)
    for b in range(nb):
        ref = _ref(M, N, rp, ci, K, A[b * M * K:(b + 1) * M * K], B[b * N * K:(b + 1) * N * K], dtype)
        _assert_matches(ref, P[b * nnz:(b + 1) * nnz])


def test_prepared_shard_survives_lazy_evictions():
    """The lazy shard cache holds 16 ranges and drops its oldest; 17 lazy builds after a prepare
    would have evicted a range kept on the same list."""
    torch = torch_cuda()
    pat, K, dtype, kw, _ = CASES["rb_f32"]
    M, N, rp, ci = pat()
    nnz = len(ci)
    plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, **kw)
    assert plan.stats()["num_row_panels"] == 33
    A = make_data(M * K)
    B = make_data(N * K)
    dA, dB, dP = _dev(torch, A, dtype), _dev(torch, B, dtype), _nan(torch, nnz)
    plan.prepare(K, panels=(0, 2))
    s0 = torch.cuda.current_stream().cuda_stream
    others = [(2 + i, 3 + i) for i in range(17)]
    for p0, p1 in others:
        plan.sddmm_panels(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), p0, p1, stream=s0)
    torch.cuda.synchronize()
    assert plan.prepared(K, panels=(0, 2))
    assert not plan.prepared(K, panels=others[0])  # the lazy list did drop its oldest
    assert plan.prepared(K, panels=others[-1])
    dP.fill_(float("nan"))
    torch.cuda.synchronize()
    g = _capture(torch, lambda s: plan.sddmm_panels(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
                                                    0, 2, stream=s))
    P = _replay(torch, g, dP, nnz)
    ref = _ref(M, N, rp, ci, K, A, B, dtype)
    mine = np.zeros(nnz, bool)
    for r in plan.array("reorderedRows")[:32]:
        mine[rp[r]:rp[r + 1]] = True
    assert mine.any() and np.isfinite(P[mine]).all() and np.isnan(P[~mine]).all()
    assert O.check_data(ref[mine], P[mine]) == 0


def test_seventeenth_prepared_range_drops_the_oldest():
    pat, K, dtype, kw, _ = CASES["rb_f32"]
    M, N, rp, ci = pat()
    plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, **kw)
    ranges = [(i, i + 1) for i in range(17)]
    for r in ranges[:16]:
        plan.prepare(K, panels=r)
    assert all(plan.prepared(K, panels=r) for r in ranges[:16])
    plan.prepare(K, panels=ranges[16])
    assert not plan.prepared(K, panels=ranges[0])
    assert all(plan.prepared(K, panels=r) for r in ranges[1:])


def _recolumn_case(pat, K, dtype, kw, delta, built, same_launch=True):
    """prepare, recolumn(delta), then the first (lazy) launch. same_launch: (K, dtype) still runs
    the launch it ran before, so its dropped layout must read as not prepared."""
    torch = torch_cuda()
    M, N, rp, ci = pat()
    nnz = len(ci)
    plan = Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=FREE, **kw)
    assert not plan.prepared(K, dtype)
    plan.prepare(K, dtype)
    assert plan.prepared(K, dtype) and built(plan.stats())
    tiles = plan.stats()["num_dense_tiles"]
    plan.recolumn(delta)
    st = plan.stats()
    assert st["num_dense_tiles"] != tiles, (tiles, st["num_dense_tiles"])  # the split did change
    # every layout that depends on the column split is gone
    assert not built(st) and st["ptile_items"] == 0 and st["rb_items"] == [0] * 5
    assert st["rb_orig_rows"] == 0 and st["rb_col_blocks"] == 0
    tile_dominated = st["num_residual"] * 4 < st["num_dense_tiles"] * 16
    if same_launch:
        assert not plan.prepared(K, dtype)
    else:  # the new split runs the column-major launch, which has nothing to build
        assert tile_dominated and dtype == F32 and plan.prepared(K, dtype)
    A = make_data(M * K)
    B = make_data(N * K)
    dA, dB, dP = _dev(torch, A, dtype), _dev(torch, B, dtype), _nan(torch, nnz)
    plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
               stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    _assert_matches(_ref(M, N, rp, ci, K, A, B, dtype), dP.cpu().numpy()[:nnz])
    assert plan.prepared(K, dtype) and built(plan.stats()) == same_launch
    return plan


def test_recolumn_drops_the_panel_tile_list():
    """bsmr_plan_recolumn rebuilds the tile list; a panel-tile item list built for the old one
    names tiles that no longer exist (found by reading Plan::build_columns, which reset the
    row-block layouts but left ptile.built set)."""
    plan = _recolumn_case(
        lambda: synth.random_rows(700, 900, 60, seed=13, zipf=1.2, empty_frac=0.05), 128, BF16,
        {"tuning": {"ptile": 1}}, 0.1, lambda st: st["ptile_items"] > 0)
    assert plan.check(128, BF16, verbose=False) == (True, "")


@pytest.mark.parametrize("delta", [0.1, 0.0])
def test_recolumn_drops_the_rowblock_layout(delta):
    """delta 0.1 keeps the pattern on the row-block launch (276 tiles, 12,108 residual entries by
    the oracle's column split): prepared before, not prepared after, correct after a lazy launch.
    delta 0.0 makes every stored column a dense-tile column (1,047 tiles, no residual): the layout
    is dropped all the same (rb_items reads 0), but fp32 K = 64 now runs the column-major launch,
    which builds nothing, so prepared() is truthfully True there."""
    pat, K, dtype, kw, built = CASES["rb_f32"]
    plan = _recolumn_case(pat, K, dtype, kw, delta, built, same_launch=delta > 0)
    assert plan.check(K, dtype, verbose=False) == (True, "")
