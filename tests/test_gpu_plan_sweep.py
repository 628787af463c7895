"""The plan builder (csrc/plan.hip k_encode / k_cluster, cluster_filter.hip) against the CPU oracle on
every row of plan_cases.PLAN_CASES, under each applicable (cluster_filter, exact_similarity)
setting: every clustering block size B = 32 .. 1024 (the reduction trees that drop warps
included), both tile sizes, the nbpr / window / tile / launch / filter-tile boundaries, rows of
dropped warps only, rows of up to 1025 column blocks, alpha at 0, below and at 0.01 and at 1, and
patterns whose similarities sit on alpha so that the exact fp32 tree decides.

Per case and setting: cluster count and all eleven plan arrays equal the oracle's, again after
recolumn to delta 0.0 and 1.1; the geometry the case is meant to reach is the one the plan
reports; the filter ran exactly where it must; tie cases made exact evaluations; the chain walked
the same pairs with and without the filter; bsmr_plan_check passes.
tests/test_plan_cases_cpu.py holds the table and the oracle to an independent float64 reference.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
import plan_cases as PC
from bsmr import Plan, tuning_from_env
from gpu_util import PLAN_ARRAYS, assert_plans_equal, oracle_plan
from plan_cases import BY_NAME, PLAN_CASES

pytestmark = pytest.mark.gpu

DELTA = 0.3
SWEEP = [(c.name, f, e) for c in PLAN_CASES for f, e in PC.settings(c)]


def _id(p):
    name, f, e = p
    return f"{name}-{'exact' if e else 'filter' + f}"


@functools.lru_cache(maxsize=2)   # the settings of one case follow each other
def oracle_of(name):
    """(csr, rows, clusters, {delta: oracle plan}) of a case, computed once for its settings."""
    c = BY_NAME[name]
    M, N, rp, ci = PC.pattern(name)
    csr, op, ncl = oracle_plan(M, N, rp, ci, c.alpha, DELTA, c.free_mem)
    rows = op.array("reorderedRows")
    plans = {DELTA: op}
    for d in (0.0, 1.1):
        plans[d] = O.Plan(csr, rows, ncl, np.float32(d))
    return csr, rows, ncl, plans


def gpu_plan(name, cluster_filter, exact):
    c = BY_NAME[name]
    M, N, rp, ci = PC.pattern(name)
    tun = None if cluster_filter is None else tuning_from_env({"BSMR_CLUSTER_FILTER": cluster_filter})
    return Plan(M, N, rp, ci, alpha=c.alpha, delta=DELTA, free_mem_bytes=c.free_mem,
                cluster_batch=c.cluster_batch, exact_similarity=exact, tuning=tun)


_EVALS = {}   # (name, filter) -> (total, exact) similarity evaluations of that run


def evals(name, cluster_filter):
    if (name, cluster_filter) not in _EVALS:
        s = gpu_plan(name, cluster_filter, False).stats()
        _EVALS[(name, cluster_filter)] = (s["total_similarity_evals"], s["exact_similarity_evals"])
    return _EVALS[(name, cluster_filter)]


@pytest.mark.parametrize("case", SWEEP, ids=_id)
def test_plan_sweep(case):
    name, cluster_filter, exact = case
    c = BY_NAME[name]
    _, rows, ncl, oplans = oracle_of(name)
    gp = gpu_plan(name, cluster_filter, exact)
    st = gp.stats()
    hdr = gp.export_rows()[0].as_dict()
    # the geometry this case is in the table for
    for k in ("block_size", "num_blocks_per_row", "cluster_block_dim"):
        assert hdr[k] == st[k] == c.ev[k], (k, hdr[k], st[k], c.ev[k])
    assert hdr["num_reordered_rows"] == PC.reordered_rows(name) == len(rows)
    assert hdr["num_zero_rows"] == c.M - len(rows)
    assert st["cluster_filter_used"] == PC.filter_expected(c, cluster_filter, exact)
    # the result
    assert st["num_clusters"] == hdr["num_clusters"] == ncl
    assert_plans_equal(gp, oplans[DELTA])
    # how it was reached
    if exact:
        # every pair on the fp32 tree, but for the pairs a zero kept norm decides (similarity 1 or
        # 0 from the integer norms alone): none of those while the tree keeps every warp
        assert 0 < st["exact_similarity_evals"] <= st["total_similarity_evals"]
        W = c.ev["cluster_block_dim"] // 32
        if W & (W - 1) == 0:
            assert st["exact_similarity_evals"] == st["total_similarity_evals"]
    else:
        _EVALS[(name, cluster_filter)] = (st["total_similarity_evals"], st["exact_similarity_evals"])
        if c.tie:
            assert st["exact_similarity_evals"] > 0
        if cluster_filter == "1":
            assert evals(name, "0") == evals(name, "1")
    ok, msg = gp.check(K=128, verbose=False)
    assert ok, msg
    for d in (0.0, 1.1):
        gp.recolumn(d)
        assert_plans_equal(gp, oplans[d])
    ok, msg = gp.check(K=128, verbose=False)
    assert ok, msg


def _first_of_each_class():
    seen = {}
    for c in PLAN_CASES:
        seen.setdefault(c.cls, c.name)
    return sorted(seen.values())


@pytest.mark.parametrize("name", _first_of_each_class())
def test_row_stage_round_trip(name):
    """One plan per class exported (bsmr_plan_export_rows) and built again from the row stage
    (bsmr_plan_import_rows, no clustering): header kept, all eleven arrays equal."""
    c = BY_NAME[name]
    M, N, rp, ci = PC.pattern(name)
    gp = gpu_plan(name, "0", False)
    hdr, rows = gp.export_rows()
    assert np.array_equal(rows, oracle_of(name)[1])
    back = Plan.from_row_stage(rp, ci, hdr, rows, delta=DELTA)
    h2 = back.export_rows()[0].as_dict()
    for k in ("M", "N", "nnz", "block_size", "num_blocks_per_row", "cluster_block_dim",
              "num_zero_rows", "num_reordered_rows", "num_clusters", "exact_similarity_evals",
              "total_similarity_evals"):
        assert h2[k] == hdr.as_dict()[k], k
    assert np.float32(h2["alpha"]) == np.float32(c.alpha)
    for a in PLAN_ARRAYS:
        assert np.array_equal(back.array(a), gp.array(a)), a
    assert_plans_equal(back, oracle_of(name)[3][DELTA])
    ok, msg = back.check(K=128, verbose=False)
    assert ok, msg
