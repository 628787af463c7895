"""GPU: the panel MFMA SDDMM (bsmr_sddmm_mfma) against the float64 sddmm_ref
straight from the CSR. P sits between two guard zones that must stay NaN and starts as NaN itself,
so an entry that is never written fails. The bound is sddmm_bound, the one every SDDMM launch is
held to. Worst RATIO on the MI355X: DESIGN.md section 23."""
import functools

import numpy as np
import pytest

import bsmr
from bsmr import BF16, F16, F32, Plan
from attention_panels_cases import block_mask
from gpu_util import half_values, to_device, torch_cuda
from sddmm_cases import assert_bound, assert_exact, grid_data, identity_data, identity_values, sddmm_ref, signed_data
from spmm_cases import entry_rows, pattern

pytestmark = pytest.mark.gpu

NAMES = ["zipf_shuffled", "empty", "hub", "block_mask"]  # every one has M, N <= 4096 (identity data)
DTYPES = [F16, BF16]
UNSUPPORTED = 6  # BSMR_ERR_UNSUPPORTED
GUARD = 64  # floats on either side of P


def pat_of(name):
    return block_mask() if name == "block_mask" else pattern(name)


def new_plan(name):
    M, N, rp, ci = pat_of(name)
    return Plan(M, N, rp, ci, alpha=0.3, delta=0.3, free_mem_bytes=288 * 1024 ** 3)


plan_of = functools.lru_cache(maxsize=None)(new_plan)


@functools.lru_cache(maxsize=None)
def operands(name, K, dtype, kind):
    """(A, B, P, S): host operands as the kernel sees them and their float64 reference."""
    pat = M, N, _, _ = pat_of(name)
    if kind == "identity":
        A, B = identity_data(M, N, K)
    elif kind == "grid":
        A, B = grid_data(M * K, 11).reshape(M, K), grid_data(N * K, 12).reshape(N, K)
    else:
        A, B = (half_values(signed_data(n * K, seed), dtype).reshape(n, K) for n, seed in ((M, 11), (N, 12)))
    return (A, B) + sddmm_ref(pat, A, B)


def new_buf(nnz):
    return torch_cuda().full((nnz + 2 * GUARD,), float("nan"), dtype=torch_cuda().float32, device="cuda")


def launch(plan, dA, dB, K, dtype, buf, stream=0):
    plan.sddmm_mfma(dA.data_ptr(), dB.data_ptr(), K, buf.data_ptr() + 4 * GUARD,
                    stream=stream or torch_cuda().cuda.current_stream().cuda_stream, dtype=dtype)


def run(plan, A, B, K, dtype, expect=None):
    """P (numpy fp32, nnz) of one launch on host operands. expect: the status the call must fail
    with, and then P must be untouched."""
    torch = torch_cuda()
    buf = new_buf(plan.nnz)
    if expect is None:
        launch(plan, to_device(A, dtype), to_device(B, dtype), K, dtype, buf)
    else:
        with pytest.raises(bsmr.BsmrError) as e:
            launch(plan, to_device(A, dtype), to_device(B, dtype), K, dtype, buf)
        assert e.value.status == expect
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.isnan(out[:GUARD]).all() and np.isnan(out[-GUARD:]).all(), "a guard zone was written"
    assert expect is None or np.isnan(out).all(), "a refused call wrote its output"
    return out[GUARD:GUARD + plan.nnz]


EXACT = [(n, 64) for n in NAMES] + [(n, K) for n in ("hub", "zipf_shuffled") for K in (32, 128, 256, 512, 1024)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,K", EXACT)
def test_exact_on_grid_data(name, K, dtype):
    plan = plan_of(name)
    A, B, P, _ = operands(name, K, F16, "grid")  # (grid values are exact in both types)
    assert_exact(run(plan, A, B, K, dtype), P, f"{name} K={K} dtype {dtype}")
    st = plan.sddmm_mfma_stats()
    assert st["fill_permille"] > 0 and (name != "hub" or st["waves"] > st["items"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [64, 512])
@pytest.mark.parametrize("name", NAMES)
def test_identity_data_puts_every_entry_at_its_own_position(name, K, dtype):
    A, B, _, _ = operands(name, K, F16, "identity")
    assert_exact(run(plan_of(name), A, B, K, dtype), identity_values(pat_of(name)), f"identity {name} K={K} dtype {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,K", [(n, 64) for n in NAMES] + [("hub", 1024)])
def test_signed_data_within_the_sddmm_bound(name, K, dtype):
    A, B, P, S = operands(name, K, dtype, "signed")
    assert_bound(run(plan_of(name), A, B, K, dtype), P, S, K, f"{name} K={K} dtype {dtype}", "sddmm_mfma")


@pytest.mark.parametrize("dtype", DTYPES)
def test_prepared_and_lazy_plans_give_equal_bits(dtype):
    name, K = "hub", 128
    A, B, _, _ = operands(name, K, dtype, "signed")
    lazy, prepared = new_plan(name), new_plan(name)
    assert not prepared.sddmm_mfma_prepared(K) and prepared.sddmm_mfma_stats()["items"] == 0
    prepared.prepare_sddmm_mfma(K)
    assert prepared.sddmm_mfma_prepared(K) and not prepared.spmm_panels_prepared(K, 1)  # (no SpMM scratch)
    P = run(lazy, A, B, K, dtype)
    assert np.array_equal(P, run(lazy, A, B, K, dtype)) and np.array_equal(P, run(prepared, A, B, K, dtype))
    assert lazy.sddmm_mfma_stats() == prepared.sddmm_mfma_stats()


@pytest.mark.parametrize("first", ["spmm_panels", "sddmm_mfma"])
def test_shares_the_lists_with_spmm_panels_in_either_order(first):
    torch = torch_cuda()
    name, K = "hub", 64
    M, N, _, _ = pat_of(name)
    A, B, P, _ = operands(name, K, F16, "signed")
    plan, dB = new_plan(name), to_device(B, F16)
    dV = torch.from_numpy(signed_data(plan.nnz, 5)).cuda()

    def spmm(p):
        Y = torch.full((M, K), float("nan"), dtype=torch.float32, device="cuda")
        p.spmm_panels(dV.data_ptr(), dB.data_ptr(), K, Y.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, dtype=F16)
        torch.cuda.synchronize()
        return Y.cpu().numpy()

    calls = {"spmm_panels": lambda p: spmm(p), "sddmm_mfma": lambda p: run(p, A, B, K, F16)}
    got = {k: calls[k](plan) for k in ([first] + [k for k in calls if k != first])}
    assert np.array_equal(got["sddmm_mfma"], run(plan_of(name), A, B, K, F16))
    assert np.array_equal(got["spmm_panels"], spmm(new_plan(name)))
    st = plan.spmm_panels_stats(1)
    assert {k: plan.sddmm_mfma_stats()[k] for k in ("panels", "items", "steps", "fill_permille")} == \
           {k: st[k] for k in ("panels", "items", "steps", "fill_permille")}


def test_capture_needs_a_prepared_plan_and_replays_to_the_eager_bits():
    torch = torch_cuda()
    name, K, dtype = "hub", 256, F16
    A, B, _, _ = operands(name, K, dtype, "signed")
    plan = new_plan(name)
    eager = run(plan_of(name), A, B, K, dtype)
    dA, dB, buf = to_device(A, dtype), to_device(B, dtype), new_buf(plan.nnz)
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
            launch(plan, dA, dB, K, dtype, buf, stream=stream.cuda_stream)
        caught.append(e.value.status)

    capture(refused).replay()  # the capture ends normally
    torch.cuda.synchronize()
    assert caught == [bsmr.NOT_PREPARED] and np.isnan(buf.cpu().numpy()).all()
    plan.prepare_sddmm_mfma(K)
    g = capture(lambda: launch(plan, dA, dB, K, dtype, buf, stream=stream.cuda_stream))
    for _ in range(3):
        buf.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy()[GUARD:-GUARD], eager)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_containment_is_exact(dtype):
    name, K = "hub", 64
    M, N, rp, ci = pat_of(name)
    A, B, _, _ = operands(name, K, dtype, "signed")
    plan = plan_of(name)
    P = run(plan, A, B, K, dtype)
    col, row = int(ci[int(rp[4]) + 1]), 3  # a column of a short row (the hub row stores it too); the hub row
    for X, hit in ((B, np.asarray(ci) == col), (A, entry_rows(M, rp) == row)):
        Xn = X.copy()
        Xn[col if X is B else row, K // 2 + 1] = np.nan
        Pn = run(plan, *((A, Xn) if X is B else (Xn, B)), K, dtype)
        assert np.isnan(Pn[hit]).all() and np.array_equal(Pn[~hit], P[~hit]) and 1 < hit.sum() < len(P)


def test_unsupported_dtype_and_k_leave_p_untouched():
    name = "hub"
    M, N, _, _ = pat_of(name)
    plan = plan_of(name)
    run(plan, np.zeros((M, 64), np.float32), np.zeros((N, 64), np.float32), 64, F32, expect=UNSUPPORTED)
    for bad in (48, 2048):
        run(plan, np.zeros((M, bad), np.float32), np.zeros((N, bad), np.float32), bad, F16, expect=UNSUPPORTED)


def test_autograd_forward_panels():
    torch = torch_cuda()
    from bsmr import autograd as ag
    name, K = "zipf_shuffled", 64
    A, B, _, _ = operands(name, K, F16, "signed")
    plan = plan_of(name)
    G = torch.from_numpy(signed_data(plan.nnz, 5)).cuda()
    got = {}
    for form in ("panels", "default"):
        da, db = (torch.from_numpy(x).half().cuda().requires_grad_() for x in (A, B))
        Pf = ag.sddmm(plan, da, db, forward=form)
        (Pf * G).sum().backward()
        got[form] = (Pf.detach().cpu().numpy(), da.grad, db.grad)
    assert np.array_equal(got["panels"][0], run(plan, A, B, K, F16))
    assert torch.equal(got["panels"][1], got["default"][1]) and torch.equal(got["panels"][2], got["default"][2])
    with pytest.raises(ValueError):
        ag.sddmm(plan, da.float(), db.float(), forward="panels")
