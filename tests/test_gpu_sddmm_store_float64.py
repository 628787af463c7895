"""GPU: every form of the row-block store pass against an exact reference, with the evidence of
which form ran.

tests/store_cases.py holds the table STORE_CASES (pattern, (K, dtype), tuning, the form evidence a
case must show) and the classifier that reads the evidence from the library's own tables
(gpu_util.rb_store: the debug exports bsmr_debug_rb_store and bsmr_debug_rb_pieces) and the
launch's form (gpu_util.plan_launch). Per case:

  * identity data (sddmm_cases.identity_data: every stored entry is 4096 row + column, exactly):
    P == reference bit for bit, so a misplaced, swapped, missing or doubled store fails and the
    message names the entry;
  * grid data: P == reference bit for bit;
  * signed data: within sddmm_cases.sddmm_bound (derived there, not tuned); "RATIO kind x case";
  * P lies between guard zones of a fixed bit pattern that no store may touch, and starts as NaN;
  * bsmr_plan_check passes on the launched layout;
  * sddmm_cases.check_stats holds (launch kind, kernel form, store form), and the case's form
    evidence is in what store_cases.classify finds: a layout that fell back to another form fails
    here, whatever the numbers are. "STORE case: evidence facts" is printed (DESIGN.md §5 records
    it: the largest item against outCap).

A case of form S (staged output by sortedPos) also recomputes the host rule that chose it: the
numpy run cutting on the dumped positions finds an item with more runs than threads, and no diag
bit is set. The other entry points (bsmr_sddmm_batch with three batches, bsmr_sddmm_panels over
three uneven ranges) run once per store form, between the same guard zones and with the same
check; a panel range builds its own layout, so its evidence is read per range from that layout
(bsmr_debug_rb_store_panels) and each store form must show in some range. One further case sets
BSMR_DIAG & 8192 on a sorted pattern (form S where the run table would fit) and must equal its
run-table twin bit for bit on signed data.
"""
import numpy as np
import pytest

from bsmr import Plan
from gpu_util import path_evidence, plan_launch, rb_store, torch_cuda
from sddmm_cases import assert_bound, assert_exact, pattern, plan_kwargs, reference
from store_cases import (DIAG_TWIN, STORE_BY_NAME, STORE_CASES, STORE_ENTRY_CASES, STORE_PANEL_CASES, as_case,
                         classify, host_rule)
from test_gpu_sddmm_edges import GUARD, P_GUARD_BITS, _guarded
from test_gpu_sddmm_float64 import _uneven_ranges, _written_by

pytestmark = pytest.mark.gpu

DATA = ("identity", "grid", "signed")


def _plan(case):
    M, N, rp, ci = pattern(case.pattern)
    return Plan(M, N, rp, ci, **plan_kwargs(case))


def _guarded_sddmm(plan, A, B, K, nnz, dtype, what):
    """P (numpy fp32, nnz) of one bsmr_sddmm with A, B and P between guard zones; P starts as NaN."""
    torch = torch_cuda()
    bufA, dA = _guarded(A, dtype)
    bufB, dB = _guarded(B, dtype)
    bufP = torch.full((nnz + 2 * GUARD,), P_GUARD_BITS, dtype=torch.int32, device="cuda")
    dP = bufP[GUARD:GUARD + nnz].view(torch.float32)
    dP.fill_(float("nan"))
    plan.sddmm(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
               stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    torch.cuda.synchronize()
    host = bufP.cpu().numpy()
    assert (host[:GUARD] == P_GUARD_BITS).all(), f"{what}: a store before P[0]"
    assert (host[GUARD + nnz:] == P_GUARD_BITS).all(), f"{what}: a store past P[nnz)"
    assert torch.isnan(bufA[:GUARD]).all() and torch.isnan(bufA[GUARD + dA.numel():]).all()
    assert torch.isnan(bufB[:GUARD]).all() and torch.isnan(bufB[GUARD + dB.numel():]).all()
    return host[GUARD:GUARD + nnz].view(np.float32).copy()


def _check_values(plan, case, what):
    """The three data sets through bsmr_sddmm; returns P on signed data."""
    nnz = len(pattern(case.pattern)[3])
    P = None
    for data in DATA:
        A, B, ref, S = reference(case.pattern, case.K, case.dtype, data)
        P = _guarded_sddmm(plan, A, B, case.K, nnz, case.dtype, f"{what} {data}")
        if data == "signed":
            assert_bound(P, ref, S, case.K, what, "rowblock/store")
        else:
            assert_exact(P, ref, f"{what} {data}")
    return P


def _evidence(plan, case, name):
    """(evidence, facts, dump) of the launched layout, printed."""
    dump = rb_store(plan, case.K, case.dtype)
    launch = plan_launch(plan, case.K, case.dtype)
    ev, facts = classify(dump, launch["pairs"])
    print(f"STORE {name}: {' '.join(sorted(ev))} | max entries / outCap = {facts['max_entries']} / "
          f"{facts['outCap']} = {facts['fill']:.3f}, {facts['items']} items, most runs {facts['max_runs']}")
    return ev, facts, dump, launch


@pytest.mark.parametrize("name", [c.name for c in STORE_CASES])
def test_store_case(name):
    sc = STORE_BY_NAME[name]
    case = as_case(sc)
    plan = _plan(case)
    _check_values(plan, case, name)
    ok, msg = plan.check(case.K, case.dtype, verbose=False)
    assert ok, msg
    assert not path_evidence(case, plan)
    ev, facts, dump, launch = _evidence(plan, case, name)
    assert launch["pairs"] == sc.pairs, f"{name}: launch pairs = {launch['pairs']}"
    assert sc.evidence <= ev, f"{name}: no evidence of {sorted(sc.evidence - ev)} ({facts})"
    if "S" in sc.evidence:
        # the host rule, recomputed: some item has more runs than the workgroup has threads (no
        # diag bit, outCap below 2^16), and rb_form refuses pairs without a run table even where
        # pair_min_items = 0 asks for them
        assert "diag" not in sc.tuning and dump["outCap"] < 65536
        wanted, most = host_rule(dump)
        assert not wanted and most > dump["NT"], f"{name}: the most runs of an item is {most}"
        assert sc.tuning.get("pair_min_items") == 0 and not launch["pairs"]


def test_diag_8192_equals_its_run_table_twin():
    """BSMR_DIAG & 8192 keeps the per-result positions on a sorted pattern: the only diag bit of
    this file, on top of the cases above. Same layout, same arithmetic, another store form: the
    results on signed data are the same bits."""
    name, bit = DIAG_TWIN
    sc = STORE_BY_NAME[name]
    case = as_case(sc)
    twin = case._replace(name=case.name + "_diag", tuning=dict(case.tuning, diag=bit),
                         proof=dict(case.proof, store="positions"))
    plans = {c.name: _plan(c) for c in (case, twin)}
    P = {c.name: _check_values(plans[c.name], c, c.name) for c in (case, twin)}
    assert np.array_equal(P[case.name].view(np.uint32), P[twin.name].view(np.uint32))
    assert not path_evidence(twin, plans[twin.name])
    ev, _, dump, _ = _evidence(plans[twin.name], twin, twin.name)
    assert "S" in ev
    wanted, most = host_rule(dump)
    assert wanted and most <= dump["NT"], "the run table would have fitted: only the diag bit keeps form S"
    ev, _, _, _ = _evidence(plans[case.name], case, case.name)
    assert "R" in ev


def _guard_p(n):
    """(buffer, P view of n floats, starting as NaN) between guard zones of P_GUARD_BITS."""
    torch = torch_cuda()
    buf = torch.full((n + 2 * GUARD,), P_GUARD_BITS, dtype=torch.int32, device="cuda")
    dP = buf[GUARD:GUARD + n].view(torch.float32)
    dP.fill_(float("nan"))
    return buf, dP


def _guards_intact(bufP, n, bufA, dA, bufB, dB, what):
    torch = torch_cuda()
    host = bufP.cpu().numpy()
    assert (host[:GUARD] == P_GUARD_BITS).all(), f"{what}: a store before P[0]"
    assert (host[GUARD + n:] == P_GUARD_BITS).all(), f"{what}: a store past the end of P"
    assert torch.isnan(bufA[:GUARD]).all() and torch.isnan(bufA[GUARD + dA.numel():]).all()
    assert torch.isnan(bufB[:GUARD]).all() and torch.isnan(bufB[GUARD + dB.numel():]).all()
    return host[GUARD:GUARD + n].view(np.float32).copy()


@pytest.mark.parametrize("name", STORE_ENTRY_CASES)
def test_batch_of_three(name):
    """bsmr_sddmm_batch: batch b writes P + b nnz (blockIdx.y in the store pass of either kernel)."""
    torch = torch_cuda()
    sc = STORE_BY_NAME[name]
    case = as_case(sc)
    K, dtype, nb = case.K, case.dtype, 3
    nnz = len(pattern(case.pattern)[3])
    plan = _plan(case)
    for data in DATA:
        # identity data is the same in every batch; the other two differ by batch
        ops = [reference(case.pattern, K, dtype, data, seed=b) for b in range(nb)]
        bufA, dA = _guarded(np.stack([o[0] for o in ops]), dtype)
        bufB, dB = _guarded(np.stack([o[1] for o in ops]), dtype)
        bufP, dP = _guard_p(nb * nnz)
        plan.sddmm_batch(nb, dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(),
                         stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
        torch.cuda.synchronize()
        P = _guards_intact(bufP, nb * nnz, bufA, dA, bufB, dB, f"{name} batch {data}").reshape(nb, nnz)
        for b, (_, _, ref, S) in enumerate(ops):
            if data == "signed":
                assert_bound(P[b], ref, S, K, f"{name} batch {b}", "rowblock/store/batch")
            else:
                assert_exact(P[b], ref, f"{name} batch {b} {data}")
    ok, msg = plan.check(K, dtype, verbose=False)
    assert ok, msg
    assert not path_evidence(case, plan)
    ev, facts, _, _ = _evidence(plan, case, name + " batch")
    assert sc.evidence <= ev, sorted(sc.evidence - ev)


@pytest.mark.parametrize("name", sorted(STORE_PANEL_CASES))
def test_panels_in_three_uneven_shards(name):
    """bsmr_sddmm_panels: each range writes exactly its rows' entries, and the three together P.
    A range runs a layout of its own (the range's reordered rows, whatever orig_rows says), so
    the form evidence is read per range from that layout (gpu_util.rb_store with panels: the
    export bsmr_debug_rb_store_panels, which also gives the form of the range's launch), and the
    case's panel evidence must be found among the three ranges."""
    torch = torch_cuda()
    sc = STORE_BY_NAME[name]
    case = as_case(sc)
    pat = pattern(case.pattern)
    K, dtype, nnz = case.K, case.dtype, len(pat[3])
    plan = _plan(case)
    s = torch.cuda.current_stream().cuda_stream
    ranges = _uneven_ranges(plan.stats()["num_row_panels"])
    masks = [_written_by(plan, pat, p0, p1) for p0, p1 in ranges]
    for data in DATA:
        A, B, ref, S = reference(case.pattern, K, dtype, data)
        bufA, dA = _guarded(A, dtype)
        bufB, dB = _guarded(B, dtype)
        bufP, dP = _guard_p(nnz)
        done = np.zeros(nnz, bool)
        for (p0, p1), mine in zip(ranges, masks):
            plan.sddmm_panels(dA.data_ptr(), dB.data_ptr(), K, dP.data_ptr(), p0, p1, stream=s, dtype=dtype)
            torch.cuda.synchronize()
            done |= mine
            assert np.array_equal(np.isfinite(dP.cpu().numpy()[:nnz]), done), \
                f"{name}: panels [{p0}, {p1}) did not write exactly their rows' entries"
        assert done.all()
        P = _guards_intact(bufP, nnz, bufA, dA, bufB, dB, f"{name} panels {data}")
        if data == "signed":
            assert_bound(P, ref, S, K, name + " panels", "rowblock/store/panels")
        else:
            assert_exact(P, ref, f"{name} panels {data}")
    ok, msg = plan.check(K, dtype, verbose=False)
    assert ok, msg
    found = set()
    for (p0, p1), mine in zip(ranges, masks):
        dump = rb_store(plan, K, dtype, panels=(p0, p1))
        assert int(dump["ent"][dump["real"]].sum()) == int(mine.sum()), "the range's items hold its entries"
        ev, facts = classify(dump, dump["pairs"])
        print(f"STORE {name} panels [{p0}, {p1}): {' '.join(sorted(ev))} | max entries / outCap = "
              f"{facts['max_entries']} / {facts['outCap']} = {facts['fill']:.3f}, {facts['items']} items, "
              f"most runs {facts['max_runs']}")
        if "S" in ev:  # the host rule, recomputed on the range's own positions
            wanted, most = host_rule(dump)
            assert not wanted and most > dump["NT"] and not dump["pairs"]
        found |= ev
    need = STORE_PANEL_CASES[name]
    assert need <= found, f"{name}: no panel range shows {sorted(need - found)}"
