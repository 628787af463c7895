"""No GPU: the columns side's lists of the panel attention backward, that is
bsmr.attention_panel_lists on bsmr.attention_pattern_transpose of the pattern, against a direct numpy
construction: per panel of 16 consecutive columns the ascending union of the rows that store one of
them, cut into steps of 32 with one mask per column, padding slots, items and the reduce list.
"""
import numpy as np
import pytest

import attention_bwd_cases as ABC
import bsmr
from test_gpu_attention_panels import pattern

NAMES = ["staircase37", "empty_row_and_panel", "split", "hub"]


@pytest.mark.parametrize("name", NAMES)
def test_transpose_is_the_transposed_pattern_and_an_involution(name):
    M, N, rp, ci = pattern(name)
    t = bsmr.attention_pattern_transpose(M, N, rp, ci)
    for got, want in zip(t, ABC.transpose((M, N, rp, ci))):
        assert np.array_equal(got, want)
    for got, want in zip(bsmr.attention_pattern_transpose(*t), (M, N, rp, ci)):
        assert np.array_equal(got, want)
    with pytest.raises(bsmr.BsmrError):
        bsmr.attention_pattern_transpose(M, int(ci.max()), rp, ci)  # a column >= N


@pytest.mark.parametrize("name", NAMES + ["split_T"])
def test_column_lists_against_a_direct_construction(name):
    M, N, rp, ci = ABC.transpose(pattern(name[:-2])) if name.endswith("_T") else pattern(name)
    lim = bsmr.attention_panels_limits()
    W, S = lim["step_cols"], lim["item_steps"]
    order, steps, masks, items, reds = bsmr.attention_panel_lists(*bsmr.attention_pattern_transpose(M, N, rp, ci))
    assert np.array_equal(order, np.arange(N))  # no order: a panel is 16 consecutive columns
    erows = np.repeat(np.arange(M), np.diff(rp.astype(np.int64)))
    want_items, want_reds, step0, part = [], [], 0, 0
    for col0 in range(0, N, 16):
        inside = (ci >= col0) & (ci < col0 + 16)
        union = np.unique(erows[inside])
        nsteps = -(-len(union) // W)
        for s in range(nsteps):
            real = union[s * W:(s + 1) * W]
            assert np.array_equal(steps[step0 + s, :len(real)], real)
            assert (steps[step0 + s, len(real):] == real[0]).all()  # padding repeats the step's first row
            for c in range(16):
                stored = erows[ci == col0 + c]
                bits = sum(1 << b for b, r in enumerate(real) if r in stored)
                assert masks[step0 + s, c] == bits, (col0, s, c)
        n = max(1, -(-nsteps // S))
        for k in range(n):
            want_items.append((col0, step0 + k * S, min(S, nsteps - k * S) if nsteps else 0, part + k if n > 1 else 0xFFFFFFFF))
        if n > 1:
            want_reds.append((col0, part, n, 0))
            part += n
        step0 += nsteps
    assert step0 == len(steps)
    assert np.array_equal(items, np.array(want_items, np.uint32).reshape(-1, 4))
    assert np.array_equal(reds, np.array(want_reds, np.uint32).reshape(-1, 4))
    if name == "split_T":
        assert len(reds) == 1 and reds[0, 2] == 2  # a union of 16 x 32 + 1 rows: two items
