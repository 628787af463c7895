"""The plan sweep's checker checks itself (no GPU): plan_cases.PLAN_CASES against the CPU oracle.

* the evidence columns of the table equal the oracle's geometry, and the table holds every
  clustering block size 32 .. 1024, both tile sizes and every boundary DESIGN.md section 3.1 lists;
* first_fit_f64 (numpy float64, written from the reference's source) gives the oracle's permutation
  on every clear case, and every planted / masked / long / shuffled case is clear;
* the oracle's guard-band fast path equals its exact fp32 tree on every case;
* the windows cases sit on alpha: many exact evaluations, another permutation one ulp below;
* each mutation of first_fit_f64 changes the permutation on the cases aimed at it.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
import plan_cases as PC
from plan_cases import BY_NAME, PLAN_CASES

NAMES = [c.name for c in PLAN_CASES]
WINDOWS = [c.name for c in PLAN_CASES if c.pattern == "windows"]
NON_POW2 = [W for W in range(1, 33) if W & (W - 1)]


@functools.lru_cache(maxsize=None)
def oracle(name, exact_all=False, below=False):
    """(rows, num_clusters, exact evaluations, all evaluations) of the oracle on a case."""
    c = BY_NAME[name]
    M, N, rp, ci = PC.pattern(name)
    csr = O.CSR.from_arrays(M, N, rp, ci)
    alpha = PC.alpha_below(c.alpha) if below else c.alpha
    rows, ncl, (ne, nt) = O.row_reorder(csr, np.float32(alpha), O.block_size(M, N, c.free_mem),
                                        exact_all=exact_all)
    rows.setflags(write=False)
    return rows, ncl, ne, nt


@functools.lru_cache(maxsize=None)
def f64(name, mutate=None):
    c = BY_NAME[name]
    M, N, rp, ci = PC.pattern(name)
    perm, ncl, gap = PC.first_fit_f64(M, N, rp, ci, c.bs, c.alpha, mutate=mutate)
    perm.setflags(write=False)
    return perm, ncl, gap


def changed(name, mutate):
    return not np.array_equal(f64(name, mutate)[0], f64(name)[0])


def test_kept_warps_of_the_reduction_tree():
    """reduce_sum's stride loop: every warp for a power-of-two count, else 2 of 3 at B = 96, 4 of 7
    at 224, 16 of 31 at 992 (warp 0 always)."""
    for W in range(1, 33):
        k = PC.kept_warps(32 * W)
        assert k[0] and len(k) == W
        assert k.all() == (W & (W - 1) == 0), W
    assert PC.kept_warps(96).tolist() == [True, True, False]
    assert int(PC.kept_warps(224).sum()) == 4 and int(PC.kept_warps(992).sum()) == 16
    assert [int(PC.kept_warps(32 * W).sum()) for W in (5, 6, 12, 24)] == [4, 4, 8, 16]


def test_evidence_columns_equal_the_oracle_geometry():
    for c in PLAN_CASES:
        M, N, rp, ci = PC.pattern(c.name)
        bs = O.block_size(M, N, c.free_mem)
        assert c.ev["block_size"] == bs == c.bs, c.name
        assert c.ev["num_blocks_per_row"] == -(-N // bs) == c.nbpr, c.name
        assert c.ev["cluster_block_dim"] == O.lib().orc_cluster_block_dim(c.nbpr), c.name
        assert len(ci) >= 2 and int(ci.max()) < N and M <= 600 and len(ci) <= 25000, c.name
        assert int(rp[0]) == 0 and (np.diff(rp.astype(np.int64)) >= 0).all(), c.name


def test_table_holds_every_shape_and_boundary():
    by_cls = {}
    for c in PLAN_CASES:
        by_cls.setdefault(c.cls, []).append(c)
    tree = by_cls["tree"]
    every_B = set(range(32, 1025, 32))
    for pat in ("planted", "windows"):
        assert {c.ev["cluster_block_dim"] for c in tree if c.pattern == pat} == every_B
    assert {(dict(c.args)["width"], np.float32(c.alpha)) for c in tree if c.pattern == "windows"} == \
        {(w, np.float32(a)) for w, a in PC.TIES}
    nb = {c.nbpr: c for c in by_cls["nbpr"]}
    assert nb[4736].ev["tile_clusters"] == 8 and nb[4737].ev["tile_clusters"] == 6
    assert all(c.ev["tile_clusters"] == 8 for c in PLAN_CASES if c.nbpr < 4736)
    assert {n % 4 for n in nb} == {0, 1, 2, 3}
    assert any(c.bs > 16 and c.free_mem < PC.FREE for c in by_cls["nbpr"])
    wins = {(PC.reordered_rows(c.name), c.M - PC.reordered_rows(c.name)) for c in by_cls["window"]}
    assert wins == {(R, z) for R in (63, 64, 65, 255, 256, 257, 513) for z in (0, 9)}
    tiles = {(PC.reordered_rows(c.name), c.cluster_batch) for c in by_cls["tiles"]
             if np.float32(c.alpha) == 1 and c.pattern == "planted"}
    assert tiles == {(R, b) for R in (64, 65) for b in (7, 8, 9, 24, 64)}
    assert {c.pattern for c in by_cls["tiles"]} == {"planted", "identical", "disjoint"}
    assert {np.float32(c.alpha) for c in by_cls["alpha"]} == \
        {np.float32(a) for a in (0.0, 0.005, 0.01, 1.0)}
    assert {(c.M, c.nbpr % 64) for c in by_cls["filter"]} == \
        {(M, r) for M in (127, 128, 129, 257) for r in (0, 1, 63)}
    assert {c.ev["cluster_block_dim"] // 32 for c in by_cls["masked"]} == {3, 7, 31}
    assert {"long", "shuffled"} <= set(by_cls)
    for c in by_cls["long"]:   # rows of 255 .. 1025 distinct column blocks
        M, N, rp, ci = PC.pattern(c.name)
        nblk = {len(np.unique(ci[rp[r]:rp[r + 1]] // c.bs)) for r in range(M)}
        assert set(PC.LONG_BLOCKS) <= nblk and c.nbpr >= 1147
    for c in by_cls["shuffled"]:
        M, N, rp, ci = PC.pattern(c.name)
        assert any((np.diff(ci[rp[r]:rp[r + 1]].astype(np.int64)) < 0).any() for r in range(M))


def test_settings_of_every_case():
    """Filter forced off everywhere, forced on wherever it can run, the exact tree on tie cases;
    the alpha cases below 0.01 are forced too (the filter must then stay off)."""
    for c in PLAN_CASES:
        s = PC.settings(c)
        assert ("0", False) in s, c.name
        assert PC.reordered_rows(c.name) >= 2, c.name   # the filter's other condition
        assert (("1", False) in s) == (np.float32(c.alpha) >= np.float32(0.01) or c.force_filter), \
            c.name
        assert ((None, True) in s) == c.tie, c.name
    assert PC.filter_expected(BY_NAME["alpha_0.005"], "1", False) == 0
    assert PC.filter_expected(BY_NAME["alpha_0.01"], "1", False) == 1
    assert PC.filter_expected(BY_NAME["alpha_0.01"], "0", False) == 0


@pytest.mark.parametrize("name", NAMES)
def test_first_fit_f64_equals_oracle_on_clear_cases(name):
    """Clear = the smallest |similarity - alpha| first_fit_f64 met exceeds CLEAR_GAP, far outside
    the fp32 tree's error: the two must agree. Every planted-type case must be clear."""
    c = BY_NAME[name]
    perm, ncl, gap = f64(name)
    if c.clear_expected:
        assert gap > PC.CLEAR_GAP, (name, gap)
    if gap > PC.CLEAR_GAP:
        rows = oracle(name)[0]
        assert np.array_equal(perm, rows), (name, gap, np.nonzero(perm != rows)[0][:5])
    else:
        assert c.tie or c.pattern in ("identical", "disjoint"), (name, gap)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_exact_all_equals_fast_path(name):
    fast, exact = oracle(name), oracle(name, exact_all=True)
    assert fast[1] == exact[1]
    assert np.array_equal(fast[0], exact[0])
    assert exact[2] == exact[3] == fast[3]   # exact_all: every evaluation on the fp32 tree


@pytest.mark.parametrize("name", [c.name for c in PLAN_CASES if c.tie])
def test_tie_cases_reach_the_exact_tree(name):
    """The fp32 tree decides in the tie cases: at least 32 evaluations inside the guard band."""
    assert oracle(name)[2] >= 32, oracle(name)[2:]


@pytest.mark.parametrize("name", WINDOWS)
def test_windows_cases_change_one_ulp_below_alpha(name):
    """Neighbouring windows sit on alpha: one fp32 ulp less and they join (fewer clusters, another
    permutation), so the decisions the fp32 tree makes at alpha are all visible."""
    at, below = oracle(name), oracle(name, below=True)
    assert not np.array_equal(at[0], below[0])
    assert below[1] < at[1]


@pytest.mark.parametrize("W", NON_POW2)
def test_mutation_all_warps_kept(W):
    assert changed(f"tree_planted_W{W}", "all_kept")


def test_mutation_all_warps_kept_other_classes():
    for name in ("masked_W3", "masked_W7", "masked_W31", "long_rows_W31", "shuffled_W5"):
        assert changed(name, "all_kept"), name
    for W in (1, 2, 4, 8, 16, 32):   # nothing to drop
        assert not changed(f"tree_planted_W{W}", "all_kept")


@pytest.mark.parametrize("name", [n for n in WINDOWS if BY_NAME[n].alpha == 0.5])
def test_mutation_ge_for_gt(name):
    """alpha = 0.5 is exact in fp32 and so is the similarity 2 x / 4 x of two neighbouring windows:
    `>=` takes what `>` refuses. (The other tie alphas round up in fp32, above the real ratio.)"""
    assert changed(name, "ge")


@pytest.mark.parametrize("name", WINDOWS + ["tiles_identical_alpha1", "alpha_0.0_disjoint"])
def test_mutation_unstable_dispersion_order(name):
    assert changed(name, "unstable")


@pytest.mark.parametrize("name", ["masked_W3", "masked_W7", "masked_W31"])
def test_mutation_zero_norm_rules_swapped(name):
    assert changed(name, "swap_zero")


@pytest.mark.parametrize("W", range(1, 33))
def test_mutation_plain_jaccard_and_unstable_on_planted(W):
    name = f"tree_planted_W{W}"
    assert changed(name, "jaccard"), name
    assert changed(name, "unstable"), name


def test_long_rows_pairs_hinge_on_their_tail_block():
    """long_rows where every warp is kept: each pair of long rows joins, and with the last block of
    one row's encoding removed (entry 254 .. 1024 of it, past every 256-entry chunk boundary) it
    does not: one cluster more. A builder that lost the tail of a long encoding would show."""
    c = BY_NAME["long_rows_W32"]
    M, N, rp, ci = PC.pattern(c.name)
    rp = rp.astype(np.int64)
    base = f64(c.name)[1]
    nblk = np.array([len(np.unique(ci[rp[r]:rp[r + 1]] // c.bs)) for r in range(M)])
    for nb in PC.LONG_BLOCKS:
        pair = np.nonzero(nblk == nb)[0]
        assert len(pair) == 2, nb
        cols = ci[rp[pair[1]]:rp[pair[1] + 1]]
        rows = [ci[rp[r]:rp[r + 1]] for r in range(M)]
        rows[pair[1]] = cols[cols // c.bs != (cols // c.bs).max()]
        M2, N2, rp2, ci2 = PC._csr_from_rows(M, N, rows)
        assert PC.first_fit_f64(M2, N2, rp2, ci2, c.bs, c.alpha)[1] == base + 1, nb
