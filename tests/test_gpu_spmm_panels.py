"""GPU: the panel MFMA SpMM (bsmr_spmm_panels / bsmr_spmm_t_panels) against the float64 spmm_ref
straight from the CSR. Every output sits between two guard zones that must stay NaN. panel_bound is
the bound derived in DESIGN.md section 21 (accumulation over (q + 1) n terms for q pieces, plus the
piece truncation u vmax sum|x|), never fitted."""
import functools

import numpy as np
import pytest

import bsmr
from bsmr import BF16, F16, F32, Plan
from attention_panels_cases import block_mask
from gpu_util import half_values, to_device, torch_cuda
from sddmm_cases import grid_data, signed_data
from spmm_cases import assert_exact, entry_rows, grid_values, pattern, signed_bound_tight, signed_values, spmm_ref

pytestmark = pytest.mark.gpu

NAMES = ["zipf_shuffled", "empty", "hub", "staircase", "block_mask"]
DTYPES = [F16, BF16]
UNSUPPORTED = 6  # BSMR_ERR_UNSUPPORTED
GUARD = 64  # floats on either side of Y
UNIT = {F16: 2.0 ** -22 + 2.0 ** -25, BF16: 2.0 ** -24}


def pat_of(name):
    return block_mask() if name == "block_mask" else pattern(name)


def new_plan(name):
    M, N, rp, ci = pat_of(name)
    return Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=288 * 1024 ** 3)


plan_of = functools.lru_cache(maxsize=None)(new_plan)


def launch(plan, side, dV, dX, K, dtype, buf, stream=0, panels=True):
    fn = {(1, True): plan.spmm_panels, (2, True): plan.spmm_t_panels, (1, False): plan.spmm, (2, False): plan.spmm_t}[side, panels]
    fn(dV.data_ptr(), dX.data_ptr(), K, buf.data_ptr() + 4 * GUARD, stream=stream or torch_cuda().cuda.current_stream().cuda_stream,
       dtype=dtype)


def run(plan, side, V, X, K, dtype, panels=True, expect=None):
    """Y (numpy fp32) of one launch on host operands; Y and its guard zones start as NaN. expect: the
    status the call must fail with, and then Y must be untouched."""
    torch = torch_cuda()
    rows = plan.M if side == 1 else plan.N
    buf = torch.full((rows * K + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    dV = torch.from_numpy(np.ascontiguousarray(V, np.float32)).cuda()
    if expect is None:
        launch(plan, side, dV, to_device(X, dtype), K, dtype, buf, panels=panels)
    else:
        with pytest.raises(bsmr.BsmrError) as e:
            launch(plan, side, dV, to_device(X, dtype), K, dtype, buf)
        assert e.value.status == expect
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.isnan(out[:GUARD]).all() and np.isnan(out[-GUARD:]).all(), "a guard zone was written"
    assert expect is None or np.isnan(out).all(), "a refused call wrote its output"
    return out[GUARD:-GUARD].reshape(rows, K)


def operands(name, side, K, dtype, kind):
    """(V, X) on the host as the kernel sees them: grid (exact) or signed full-mantissa data."""
    M, N, rp, _ = pat_of(name)
    n = (N if side == 1 else M) * K
    if kind == "grid":
        return grid_values(int(rp[-1]), 5), grid_data(n, 6).reshape(-1, K)
    return signed_values(int(rp[-1]), 5), half_values(signed_data(n, 6), dtype).reshape(-1, K)


def panel_bound(pat, side, V, X, ref, dtype):
    M, N, rp, ci = pat
    _, S, n = ref
    dst = entry_rows(M, rp) if side == 1 else np.asarray(ci, np.int64)
    vmax = np.zeros(len(n))
    np.maximum.at(vmax, dst, np.abs(np.asarray(V, np.float64)))
    sum_x = spmm_ref(pat, side, np.ones(len(ci)), np.abs(X))[0]
    pieces = 2 if dtype == F16 else 3
    return signed_bound_tight(S * (1 + 2.0 ** -7), (pieces + 1) * n, vmax[:, None]) + UNIT[dtype] * vmax[:, None] * sum_x


def assert_bound(Y, ref, bound, what):
    Yr, _, n = ref
    assert np.isfinite(Y).all() and (Y[n == 0] == 0).all(), what
    err = np.abs(Y.astype(np.float64) - Yr)
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"RATIO spmm_panels {ratio:.4f} {what}")
    assert (err <= bound).all(), f"{what}: worst |Y - ref| / bound = {ratio:.3f}"


EXACT = [(n, 64) for n in NAMES] + [(n, K) for n in ("zipf_shuffled", "hub") for K in (32, 128, 256, 512)] + [("hub", 1024)]


@pytest.mark.parametrize("name,K", EXACT)
def test_exact_on_grid_data(name, K):
    pat, plan = pat_of(name), plan_of(name)
    for side in (1, 2):
        V, X = operands(name, side, K, F16, "grid")
        ref = spmm_ref(pat, side, V, X)
        for dtype in DTYPES:
            assert_exact(run(plan, side, V, X, K, dtype), ref, f"{name} K={K} side {side} dtype {dtype}")
    if name == "hub":
        assert plan.spmm_panels_stats(1)["split_panels"] > 0 and plan.spmm_panels_stats(2)["fill_permille"] > 0


@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["zipf_shuffled", "hub"])
def test_scaling_v_by_a_power_of_two_scales_y_exactly(name, dtype, side):
    pat, plan = pat_of(name), plan_of(name)
    V, X = operands(name, side, 64, dtype, "signed")
    Yr, S, _ = spmm_ref(pat, side, V, X)
    # the float64 reference of every case stays inside fp32's normal range
    assert S.max() * 2.0 ** 40 < 2.0 ** 127 and np.abs(Yr[Yr != 0]).min() * 2.0 ** -40 > 2.0 ** -126
    Y0 = run(plan, side, V, X, 64, dtype)
    for k in (-40, -20, 20, 40):
        Yk = run(plan, side, V * np.float32(2.0 ** k), X, 64, dtype)
        assert np.array_equal(Yk, Y0 * np.float32(2.0 ** k)), f"{name} side {side} dtype {dtype} k={k}"


@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("direction", [1, -1], ids=["ascending", "descending"])
def test_mixed_magnitudes_in_one_row(direction, dtype, side):
    """Exponents 2^-30 .. 2^30 along the union (ascending source index): the running scale grows
    late (ascending) or is set by the first step (descending). hub: split panels on side 1."""
    pat, plan = pat_of("hub"), plan_of("hub")
    M, N, rp, ci = pat
    V, X = operands("hub", side, 64, dtype, "signed")
    src, nsrc = (np.asarray(ci, np.int64), N) if side == 1 else (entry_rows(M, rp), M)
    V = V * np.exp2(direction * np.round(-30 + 60 * src / (nsrc - 1))).astype(np.float32)
    ref = spmm_ref(pat, side, V, X)
    assert_bound(run(plan, side, V, X, 64, dtype), ref, panel_bound(pat, side, V, X, ref, dtype),
                 f"mixed hub side {side} dtype {dtype} direction {direction}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_signed_data_within_the_bound_and_of_the_gather_form(name, dtype):
    pat, plan = pat_of(name), plan_of(name)
    for side in (1, 2):
        V, X = operands(name, side, 64, dtype, "signed")
        ref = spmm_ref(pat, side, V, X)
        bound = panel_bound(pat, side, V, X, ref, dtype)
        Y = run(plan, side, V, X, 64, dtype)
        assert_bound(Y, ref, bound, f"{name} side {side} dtype {dtype}")
        Yg = run(plan, side, V, X, 64, dtype, panels=False)
        assert (np.abs(Y.astype(np.float64) - Yg) <= bound + signed_bound_tight(ref[1], ref[2])).all()


@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_properties(dtype, side):
    name, K = "hub", 64
    pat = M, N, rp, ci = pat_of(name)
    V, X = operands(name, side, K, dtype, "signed")
    lazy, prepared = new_plan(name), new_plan(name)
    assert not prepared.spmm_panels_prepared(K, side) and prepared.spmm_panels_stats(side)["items"] == 0
    prepared.prepare_spmm_panels(K, side)
    assert prepared.spmm_panels_prepared(K, side) and not prepared.spmm_panels_prepared(K, 3 - side)
    Y = run(lazy, side, V, X, K, dtype)
    assert np.array_equal(Y, run(lazy, side, V, X, K, dtype)) and np.array_equal(Y, run(prepared, side, V, X, K, dtype))
    e = int(rp[4]) + 7  # a NaN in one V[e]: exactly its destination, all of it
    dst, src = (entry_rows(M, rp)[e], int(ci[e])) if side == 1 else (int(ci[e]), entry_rows(M, rp)[e])
    Vn = V.copy()
    Vn[e] = np.nan
    Yn = run(lazy, side, Vn, X, K, dtype)
    hit = np.zeros(len(Y), bool)
    hit[dst] = True
    assert np.isnan(Yn[hit]).all() and np.array_equal(Yn[~hit], Y[~hit])
    # a NaN dense row: every destination of the panels whose union holds it, and no other
    lists = (bsmr.attention_panel_lists(M, N, rp, ci, lazy.array("reorderedRows")) if side == 1
             else bsmr.attention_panel_lists(*bsmr.attention_pattern_transpose(M, N, rp, ci)))
    rows, cols, _, items, _ = lists
    hit[:] = False
    for row0, step0, nsteps, _ in items.astype(np.int64):
        if (cols[step0:step0 + nsteps] == src).any():
            hit[rows[row0:row0 + 16]] = True
    Xn = X.copy()
    Xn[src] = np.nan
    Yn = run(lazy, side, V, Xn, K, dtype)
    assert np.isnan(Yn[hit]).all() and np.array_equal(Yn[~hit], Y[~hit]) and 0 < hit.sum() < len(Y)
    assert (run(lazy, side, np.zeros_like(V), X, K, dtype) == 0).all()
    run(lazy, side, V, X, K, F32, expect=UNSUPPORTED)
    for bad in (48, 2048):
        run(lazy, side, V, np.zeros(((N if side == 1 else M), bad), np.float32), bad, dtype, expect=UNSUPPORTED)


@pytest.mark.parametrize("side", [1, 2])
def test_capture_needs_a_prepared_plan_and_replays_to_the_same_bits(side):
    torch = torch_cuda()
    name, K, dtype = "hub", 128, F16
    V, X = operands(name, side, K, dtype, "signed")
    plan = new_plan(name)
    eager = run(plan_of(name), side, V, X, K, dtype)
    dV, dX = torch.from_numpy(V).cuda(), to_device(X, dtype)
    buf = torch.full((eager.size + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    stream, caught = torch.cuda.Stream(), []
    torch.cuda.synchronize()

    def capture(body):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            body()
        return g

    def refused():
        buf.fill_(float("nan"))
        with pytest.raises(bsmr.BsmrError) as e:
            launch(plan, side, dV, dX, K, dtype, buf, stream=stream.cuda_stream)
        caught.append(e.value.status)

    capture(refused).replay()  # the capture ends normally
    assert caught == [bsmr.NOT_PREPARED]
    plan.prepare_spmm_panels(K, side)
    g = capture(lambda: launch(plan, side, dV, dX, K, dtype, buf, stream=stream.cuda_stream))
    for _ in range(3):
        buf.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy()[GUARD:-GUARD].reshape(eager.shape), eager)


@pytest.mark.parametrize("first", ["spmm", "attention"])
def test_rows_side_shares_the_attention_lists(first):
    torch = torch_cuda()
    name, K = "zipf_shuffled", 64
    M, N, _, _ = pat_of(name)
    V, X = operands(name, 1, K, F16, "signed")
    plan = new_plan(name)
    Q, KV = to_device(np.ones((M, K), np.float32), F16), to_device(X, F16)
    O = torch.empty((M, K), dtype=torch.float32, device="cuda")

    def attention(p):
        p.attention_panels(Q.data_ptr(), KV.data_ptr(), KV.data_ptr(), K, K, O.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream, dtype=F16)
        torch.cuda.synchronize()
        return O.cpu().numpy()

    if first == "attention":
        attention(plan)
    Y = run(plan, 1, V, X, K, F16)
    assert np.array_equal(Y, run(plan_of(name), 1, V, X, K, F16))
    assert np.array_equal(attention(plan), attention(new_plan(name)))
    st = plan.attention_panels_stats()
    assert plan.spmm_panels_stats(1) == {k: st[k] for k in plan.spmm_panels_stats(1)}


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_backward_panels(dtype):
    """A.grad and B.grad of sum(G . sddmm(A, B)) against the float64 dense masked computation,
    relative to its largest element: at most 8 x the error of the same dense computation in the
    operand type on the CPU (section 18's end-to-end rule). "gather" stays what Plan.spmm gives."""
    torch = torch_cuda()
    from bsmr import autograd as ag
    name, K = "zipf_shuffled", 64
    pat = M, N, rp, ci = pat_of(name)
    plan, tdt = plan_of(name), {F16: torch.float16, BF16: torch.bfloat16}[dtype]
    G, A = operands(name, 2, K, dtype, "signed")
    _, B = operands(name, 1, K, dtype, "signed")
    Gd = np.zeros((M, N))
    Gd[entry_rows(M, rp), ci] = G
    want = {"A": Gd @ B.astype(np.float64), "B": Gd.T @ A.astype(np.float64)}
    ta, tb = (torch.from_numpy(x).to(tdt).requires_grad_() for x in (A, B))
    ((ta @ tb.T) * torch.from_numpy(Gd).to(tdt)).sum().backward()
    cpu = {"A": ta.grad.double().numpy(), "B": tb.grad.double().numpy()}
    got = {}
    for form in ("panels", "gather"):
        da, db = (torch.from_numpy(x).to(tdt).cuda().requires_grad_() for x in (A, B))
        (ag.sddmm(plan, da, db, backward=form) * torch.from_numpy(G).cuda()).sum().backward()
        got[form] = {"A": da.grad, "B": db.grad}
    for side, k in ((1, "A"), (2, "B")):
        top = np.abs(want[k]).max()
        cpu_err, gpu_err = (np.abs(x - want[k]).max() / top for x in (cpu[k], got["panels"][k].double().cpu().numpy()))
        print(f"AUTOGRAD d{k} dtype {dtype}: CPU {cpu_err:.3e} GPU {gpu_err:.3e}")
        assert gpu_err <= 8 * cpu_err
        Yg = run(plan, side, G, B if side == 1 else A, K, dtype, panels=False)
        assert torch.equal(got["gather"][k].cpu(), torch.from_numpy(Yg).to(tdt))
    with pytest.raises(ValueError):
        ag.sddmm(plan, da.float(), db.float(), backward="panels")
