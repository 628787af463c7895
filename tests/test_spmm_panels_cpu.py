"""Host only: bsmr_spmm_panel_positions, where in V the panel SpMM finds the entry behind every set
mask bit (csrc/spmm_panels.cpp), against a direct numpy construction: for every set bit of every
step, in step / panel row / bit order, the CSR index of (row, column). Both sides of patterns with
unsorted CSR rows and M % 16 != 0 (zipf_shuffled), empty rows and columns, a split panel (hub: a
2,048-column row), every list length (staircase) and the 16 x 16 block mask."""
import numpy as np
import pytest

import bsmr
from attention_panels_cases import block_mask
from spmm_cases import entry_rows, pattern

NAMES = ["zipf_shuffled", "empty", "hub", "staircase", "block_mask"]
INVALID = 1  # BSMR_ERR_INVALID, as bsmr_attention_panel_lists reports bad input


def pat_of(name):
    return block_mask() if name == "block_mask" else pattern(name)


def side_lists(pat, side, order=()):
    M, N, rp, ci = pat
    if side == 1:
        return bsmr.attention_panel_lists(M, N, rp, ci, order)
    return bsmr.attention_panel_lists(*bsmr.attention_pattern_transpose(M, N, rp, ci))


def expected(pat, side, lists):
    M, N, rp, ci = pat
    rows, cols, masks, items, _ = lists
    s, r, c = np.nonzero((masks[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1)  # step, row, bit order
    row0 = np.repeat(items[:, 0], items[:, 2]).astype(np.int64)  # steps follow the items
    dst, src = rows[row0[s] + r].astype(np.int64), cols[s, c].astype(np.int64)
    i, j = (dst, src) if side == 1 else (src, dst)
    keys = entry_rows(M, rp) * N + ci.astype(np.int64)
    by_key = np.argsort(keys)
    at = np.searchsorted(keys[by_key], i * N + j)
    assert (keys[by_key][at] == i * N + j).all()
    counts = np.bincount(s * 16 + r, minlength=16 * len(cols))
    return (np.cumsum(counts) - counts).reshape(-1, 16), by_key[at]


@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_positions_match_the_csr(name, side):
    pat = pat_of(name)
    M, N, rp, ci = pat
    order = np.random.default_rng(3).permutation(M)[:M - 5] if side == 1 else ()  # a launch order that names most rows
    lists = side_lists(pat, side, order)
    base, pos = bsmr.spmm_panel_positions(M, N, rp, ci, side, lists)
    want_base, want_pos = expected(pat, side, lists)
    assert np.array_equal(pos, want_pos) and np.array_equal(base, want_base)
    assert np.array_equal(np.sort(pos), np.arange(len(ci)))  # every position exactly once
    assert len(lists[4]) > 0 or (name, side) != ("hub", 1)  # the hub row's panel is split


@pytest.mark.parametrize("what", ["rowptr_descends", "column_past_N", "other_pattern", "bit_dropped", "side"])
def test_invalid_input_is_refused(what):
    M, N, rp, ci = pattern("empty")
    lists = list(side_lists((M, N, rp, ci), 1))
    rp, ci, side = rp.copy(), ci.copy(), 1
    if what == "rowptr_descends":
        rp[3] = rp[4] + 1
    elif what == "column_past_N":
        ci[0] = N
    elif what == "other_pattern":
        row = int(np.nonzero(np.diff(rp))[0][0])  # the first stored entry moves to a column its row does not hold
        ci[rp[row]] = next(c for c in range(N) if c not in set(ci[rp[row]:rp[row + 1]].tolist()))
    elif what == "bit_dropped":
        masks = lists[2].copy()
        s, r = np.argwhere(masks)[0]
        masks[s, r] &= masks[s, r] - 1
        lists[2] = masks
    else:
        side = 3
    with pytest.raises(bsmr.BsmrError) as e:
        bsmr.spmm_panel_positions(M, N, rp, ci, side, lists)
    assert e.value.status == INVALID
