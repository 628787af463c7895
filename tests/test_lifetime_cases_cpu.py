"""CPU: the tables of tests/lifetime_cases.py can do what tests/test_gpu_plan_lifetime.py claims for
them. The sequences are deterministic; every operation of every family, every refused call, every
delta, every growth and every order of first use occurs; the model follows the header's rules on
hand-checked prefixes; the bit comparison rejects one ulp, the sign of a zero and a NaN payload."""
import numpy as np
import pytest

import lifetime_cases as LC
import spmm_cases as PC
from bsmr import BF16, F32
from lifetime_cases import arg, st

HAND = LC.hand_written()


def facts(kind="rowblock", pattern="hub"):
    """A plan as the model sees it, written by hand: the `hub` pattern (67 rows of 1 - 3 entries
    but row 3, which holds all 2048 columns; no column holds more than 3), 5 row panels, its own
    SDDMM at (128, bf16) running `kind`, and a row-block slot for every fp32 row size used."""
    pat = PC.pattern(pattern)
    launch = {}
    for d in LC.DELTAS:
        launch[(d, 128, BF16)] = (kind, 1 if kind in ("rowblock", "dense") else -1)
        launch[(d, 128, F32)] = ("rowblock", 2)
        launch[(d, 32, F32)] = ("rowblock", 0)
        launch[(d, 64, F32)] = ("rowblock", 1)
    assert set(launch) == set(LC.launch_keys(128, BF16))
    return LC.Facts("by_hand", pat, 128, BF16, 5, launch)


def after(steps, f=None):
    return LC.run_model(f or facts(), steps)[0]


def launches(steps, family):
    return [i for i, s in enumerate(steps) if s.family == family and s.op in LC.LAUNCHES]


# --------------------------------------------------------------------------- the tables ----
def test_sequences_are_deterministic():
    assert LC.hand_written() == HAND
    for seed in LC.RANDOM_SEEDS:
        a, b = LC.random_sequence(seed), LC.random_sequence(seed)
        assert a == b and len(a) == LC.RANDOM_LENGTH + len(LC.CODA)
    assert len({tuple(LC.random_sequence(s)) for s in LC.RANDOM_SEEDS}) == len(LC.RANDOM_SEEDS)
    assert all(seq[-len(LC.CODA):] == LC.CODA for seq in HAND.values())


def test_every_operation_of_every_family_occurs():
    steps = [s for seq in HAND.values() for s in seq]
    seen = {(s.family, s.op) for s in steps}
    for family, ops in LC.OPS.items():
        for op in ops:
            assert (family, op) in seen, (family, op)
            if op in LC.LAUNCHES and op != "panels_one":  # both data sets
                assert {arg(s, "data") for s in steps if (s.family, s.op) == (family, op)} == {"exact", "signed"}, op
        assert {arg(s, "what") for s in steps if s.family == family and s.op == "refused"} == set(LC.REFUSED[family])
    assert {arg(s, "delta") for s in steps if s.op == "recolumn"} == set(LC.DELTAS)
    assert {arg(s, "want") for s in steps if s.op == "attention_backward"} == set(LC.SUBSETS) and len(LC.SUBSETS) == 7
    assert {arg(s, "lse") for s in steps if s.op == "attention"} == {True, False}
    for op in LC.OPS["heads"]:
        got = {LC.HEADS_BH[arg(s, "bh")] for s in steps if s.op == op}
        assert got == {(1, 3), (2, 2), (1, 1)}, (op, got)
    assert {arg(s, "chunk") for s in steps if s.op == "prepare_spmm"} >= {0, 32}
    assert {arg(s, "local") for s in steps if s.op == "prepare_panels"} == {True, False}
    assert {arg(s, "i") for s in steps if s.op == "panels_one"} == set(range(LC.N_CACHE_RANGES))
    for family in LC.FAMILIES:  # the same holds for what the random sequences draw from
        assert {s.op for s in LC.pool() if s.family == family} >= set(LC.OPS[family]) | {"refused"}


def test_every_ordered_pair_of_families_is_built_in_that_order_somewhere():
    first = {name: {f: min(i for i, s in enumerate(seq) if s.family == f) for f in LC.FAMILIES
                    if any(s.family == f for s in seq)} for name, seq in HAND.items()}
    for a in LC.FAMILIES:
        for b in LC.FAMILIES:
            if a != b:
                assert any(a in f and b in f and f[a] < f[b] for f in first.values()), (a, b)
    # and the backward is built both after the forward (it borrows the row lists) and before (it owns them)
    f = facts()
    assert LC.run_model(f, HAND["first_use_forward"])[0].bwd["shared"] is True
    assert LC.run_model(f, HAND["first_use_reverse"])[0].bwd["shared"] is False


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_a_recolumn_and_every_refused_call_between_two_uses(family):
    def between(pred):
        for seq in HAND.values():
            use = launches(seq, family)
            hits = [i for i, s in enumerate(seq) if pred(s)]
            if any(use and use[0] < i < use[-1] for i in hits):
                return True
        return False

    assert between(lambda s: s.op == "recolumn")
    for what in LC.REFUSED[family]:
        assert between(lambda s: s.family == family and s.op == "refused" and arg(s, "what") == what), what


def test_every_growth_occurs():
    f = facts()
    conc = {name: LC.run_model(f, seq)[1] for name, seq in HAND.items()}

    def in_order(values, want):
        it = iter(values)
        return all(any(v == w for v in it) for w in want)

    def some(op_filter, key, want):
        return any(in_order([key(c) for c in seq if op_filter(c)], want) for seq in conc.values())

    spmm = lambda c: c.op in ("spmm", "spmm_t", "sddmm_backward")  # noqa: E731
    assert some(spmm, lambda c: arg(c, "K"), [16, 64])
    assert some(lambda c: c.op == "prepare_spmm", lambda c: arg(c, "chunk"), [0, 32, 0])
    assert some(lambda c: c.op == "attention", lambda c: arg(c, "Dv"), [48, 64])
    fwd = lambda c: c.op in ("attention", "attention_heads")  # noqa: E731
    bwd = lambda c: c.op in ("attention_backward", "attention_backward_heads")  # noqa: E731
    assert some(fwd, lambda c: arg(c, "slices"), [1, 4, 1])
    assert some(bwd, lambda c: arg(c, "slices"), [1, 4, 1])
    # the SpMM chunk changes between two sddmm_backward calls, in both directions
    seq = conc["spmm_chunk_change"]
    m, chunks = LC.Model(f), []
    for c in seq:
        m.apply(c)
        if c.op == "sddmm_backward":
            chunks.append(m.spmm[1]["chunk"])
    assert in_order(chunks, [PC.DEFAULT_CHUNK, 32, PC.DEFAULT_CHUNK])
    # seventeen distinct single-range layouts, none the whole plan: one more than a cache holds
    for P in (5, 19, 33, 128):
        r = LC.cache_ranges(P)
        assert len(set(r)) == LC.N_CACHE_RANGES == LC.MAX_RANGES + 1
        assert all(0 <= p0 < p1 <= P and (p0, p1) != (0, P) for _, p0, p1 in r)
    m = after(HAND["first_use_forward"])
    assert m.largest == dict(spmm_K=64, attn_Dv=64, attn_slices=4, bwd_slices=4)


def test_projection_keeps_the_family_and_every_recolumn():
    seq = HAND["recolumn_between"]
    for family in LC.FAMILIES:
        p = LC.projection(seq, family)
        assert [s for s in p if s.op == "recolumn"] == [s for s in seq if s.op == "recolumn"]
        assert {s.family for s in p} == {family, "plan"}
        assert [s for s in p if s.family == family] == [s for s in seq if s.family == family]


def test_every_sequence_resolves_on_every_kind_of_plan():
    """concrete() and the model run through every sequence, whatever the plan launches; a plan
    without any row-block slot gets the plain panel launch where the local one was asked for."""
    for kind in ("rowblock", "dense", "ptile", "half", "colmajor"):
        f = facts(kind)
        for seq in list(HAND.values()) + [LC.random_sequence(s) for s in LC.RANDOM_SEEDS]:
            m, conc = LC.run_model(f, seq)
            assert len(conc) == len(seq) and set(m.prepared().values()) <= {True, False}
            assert not any(arg(c, "substituted") for c in conc)  # (fp32 has a slot at every row size here)
    f = facts("half")
    none = f._replace(launch={k: (v[0], -1) for k, v in f.launch.items()})
    conc = LC.run_model(none, HAND["first_use_forward"])[1]
    assert not any(c.op == "panels_local" for c in conc)
    assert any(arg(c, "substituted") for c in conc)
    assert all(arg(c, "dtype") == F32 for c in conc if c.family == "panels" and c.op != "refused")


# ---------------------------------------------------------------------------- the model ----
def test_model_sddmm_layouts_by_launch_kind():
    own, f32 = ("sddmm", 128, BF16), ("sddmm", 128, F32)
    m = after([])
    assert not m.answer(own) and not m.answer(f32) and not any(m.prepared().values())
    assert after([st("sddmm", "stats")]).prepared() == m.prepared()  # stats() is an observer
    for op in ("sddmm", "sddmm_batch", "prepare", "check"):  # check(K, dtype) builds what a launch would
        m = after([st("sddmm", op, data="exact")])
        assert m.answer(own) and not m.answer(f32), op
        m.apply(LC.recolumn(1.1))  # the row-block layouts depend on the column split
        assert not m.answer(own)
    for kind, before, kept in (("dense", False, True), ("ptile", False, False), ("half", True, True),
                               ("colmajor", True, True)):
        f = facts(kind)
        assert after([], f).answer(own) is before, kind  # the column-major lists are the plan's own
        m = after([st("sddmm", "check")], f)
        assert m.answer(own)
        m.apply(LC.recolumn(0.0))  # the dense-sampled list depends on S only and stays
        assert m.answer(own) is kept, kind


def test_model_panel_ranges_and_their_two_caches():
    f = facts()
    r = LC.uneven_ranges(f.P)
    assert r == [(0, 1), (1, 2), (2, 5)]
    key = lambda i, local=False: ("panels", 128, BF16) + r[i] + (local,)  # noqa: E731
    m = after([st("panels", "prepare_panels", r=0, local=False)])
    assert m.answer(key(0)) and not m.answer(key(1)) and not m.answer(key(0, True))  # no identity row list yet
    steps = [st("panels", "prepare_panels", r=0, local=False), st("panels", "panels", data="exact")]
    m = after(steps)
    assert all(m.answer(key(i)) for i in range(3)) and len(m.prep) == 1 and len(m.lazy) == 2
    m = after(steps + [st("panels", "panels_local", data="exact")])
    assert all(m.answer(key(i, True)) for i in range(3))
    # seventeen lazy ranges turn the lazy cache over; a prepared range is never evicted
    turn = steps + [st("panels", "panels_one", i=i, data="exact") for i in range(LC.N_CACHE_RANGES)]
    m = after(turn)
    assert m.answer(key(0)) and not m.answer(key(1)) and not m.answer(key(2)) and len(m.lazy) == LC.MAX_RANGES
    cr = LC.cache_ranges(5)
    one = lambda i: ("panels",) + LC.PANEL_KD[cr[i][0]] + cr[i][1:] + (False,)  # noqa: E731
    assert not m.answer(one(0)) and m.answer(one(1)) and m.answer(one(16))
    # a lazy range that is prepared later moves to the prepared list
    m = after(steps[::-1])
    assert len(m.prep) == 1 and len(m.lazy) == 2 and m.answer(key(0))
    # recolumn drops both caches and keeps the identity row list
    m = after(turn + [st("panels", "panels_local", data="exact"), LC.recolumn(0.0)])
    assert not any(m.answer(key(i)) for i in range(3)) and m.iota and not m.prep and not m.lazy


def test_model_spmm_sides_chunk_and_scratch():
    q = lambda K, sides: ("spmm", K, sides)  # noqa: E731
    m = after([st("spmm", "spmm", kd=0, data="exact")])
    # rows: the 2048 row has 16 partial rows at the default chunk, so K = 64 needs a larger scratch
    assert m.answer(q(16, 1)) and not m.answer(q(64, 1)) and not m.answer(q(16, 2)) and not m.answer(q(16, 3))
    assert m.stats()["spmm1"] == dict(segments=66 + 16, split_dsts=1, partials=16, max_list=2048, chunk=128)
    assert m.stats()["spmm2"]["chunk"] == 0
    # columns: none is split, so any K is covered once the lists exist
    m = after([st("spmm", "spmm_t", kd=0, data="exact")])
    assert m.answer(q(64, 2)) and m.stats()["spmm2"]["partials"] == 0
    m = after([st("spmm", "sddmm_backward", kd=0, data="exact"), st("spmm", "prepare_spmm", kd=1, sides=3, chunk=32)])
    assert all(m.answer(q(K, s)) for K in (16, 64) for s in (1, 2, 3)) and m.stats()["spmm1"]["partials"] == 64
    m.apply(LC.concrete(st("spmm", "prepare_spmm", kd=0, sides=3, chunk=0), facts(), 0.3))  # 0 keeps the lists
    assert m.stats()["spmm1"]["chunk"] == 32 and m.answer(q(64, 1))
    # another non-zero chunk rebuilds the lists; the new scratch covers this call's K = 16 only
    m.apply(LC.concrete(st("spmm", "prepare_spmm", kd=0, sides=1, chunk=128), facts(), 0.3))
    assert m.stats()["spmm1"]["chunk"] == 128 and m.answer(q(16, 1)) and not m.answer(q(64, 1))
    m.apply(LC.recolumn(1.1))  # the lists depend on S and the row order only
    assert m.answer(q(16, 3))


def test_model_attention_scratch_covers_the_largest_product_so_far():
    a, b = lambda D, Dv, z: ("attn", D, Dv, z), lambda D, Dv, z: ("bwd", D, Dv, z)  # noqa: E731
    m = after([st("attn", "attention", cfg=0, data="exact", lse=True)])
    # 8 partials (2048 / 256): 8 x 50 floats cover (32, 48) at one slice and nothing larger
    assert m.answer(a(32, 48, 1)) and not m.answer(a(64, 64, 1)) and not m.answer(a(32, 48, 3))
    m.apply(LC.concrete(st("heads", "attention_heads", cfg=0, data="exact", bh=0), facts(), 0.3))
    # three slices at Dv = 48 hold 1200 floats: enough for one slice at Dv = 64 (528), not for three (1584)
    assert m.answer(a(64, 64, 1)) and m.answer(a(32, 48, 3)) and not m.answer(a(64, 64, 3)) and not m.answer(a(32, 48, 4))
    assert not m.answer(b(32, 48, 1)) and m.stats()["bwd"]["row_segments"] == 0
    m.apply(LC.concrete(st("attn_bwd", "attention_backward", cfg=0, data="exact", want=("GQ",)), facts(), 0.3))
    assert m.bwd["shared"] and m.answer(b(32, 48, 1)) and not m.answer(b(64, 64, 1)) and not m.answer(b(32, 48, 3))
    assert m.stats()["bwd"]["delta_bytes"] == 4 * 67 and m.stats()["bwd"]["row_scratch_bytes"] == 4 * 8 * 32
    assert m.stats()["bwd"]["col_scratch_bytes"] == 0  # no column of `hub` is split
    m.apply(LC.concrete(st("heads", "attention_backward_heads", cfg=1, data="exact", bh=1, want=("GK",)), facts(), 0.3))
    assert all(m.answer(b(D, Dv, z)) for D, Dv, _ in LC.SHAPES for z in (1, 3, 4))
    assert m.stats()["bwd"]["delta_bytes"] == 4 * 4 * 67 and m.stats()["attn"]["split_rows"] == 1
    before = (m.prepared(), m.stats())
    for family in LC.FAMILIES:  # a refused call changes nothing, and neither does recolumn here
        for what in LC.REFUSED[family]:
            m.apply(LC.refused(family, what))
    m.apply(LC.recolumn(0.0))
    assert (m.prepared(), m.stats()) == before
    # `zipf` splits columns instead (16 of them, 35 partials): that scratch is (D + Dv) wide; built
    # before any forward, the backward owns its row lists, and a later forward does not change that
    m = after([st("attn_bwd", "attention_backward", cfg=1, data="exact", want=("GV",)),
               st("attn", "attention", cfg=1, data="exact", lse=True)], facts(pattern="zipf"))
    assert not m.bwd["shared"] and m.stats()["bwd"]["col_scratch_bytes"] == 4 * 35 * (64 + 64)
    assert m.stats()["bwd"]["row_scratch_bytes"] == 0 and m.stats()["bwd"]["col_split"] == 16


def test_model_softmax():
    m = after([])
    assert not m.answer(("softmax",)) and m.stats()["softmax"]["items"] == 0 and m.stats()["softmax"]["wave_max"] > 0
    for op in LC.OPS["softmax"]:
        m = after([st("softmax", op, data="exact")])
        assert m.answer(("softmax",)) and m.stats()["softmax"]["block_rows"] == 1
        m.apply(LC.recolumn(1.1))
        assert m.answer(("softmax",))


# ------------------------------------------------------------------- the bit comparison ----
def test_bit_comparison_rejects_one_ulp_a_zero_sign_and_a_nan_payload():
    x = np.array([[1.0, -0.0, np.nan, 0.0], [3.5, np.inf, -np.inf, 2.0 ** -140]], np.float32)
    assert LC.same_bits(x, x.copy())
    LC.assert_same_bits(x, x.copy(), "copy")
    ulp = x.copy()
    ulp[0, 0] = np.nextafter(np.float32(1.0), np.float32(2.0))
    zero = x.copy()
    zero[0, 1] = 0.0
    payload = x.copy()
    payload.view(np.uint32)[0, 2] ^= 1
    # (a comparison of values sees neither of the last two)
    assert np.isnan(payload[0, 2])
    assert np.array_equal(x, zero, equal_nan=True) and np.array_equal(x, payload, equal_nan=True)
    for name, y in (("ulp", ulp), ("zero", zero), ("payload", payload)):
        assert not LC.same_bits(x, y), name
        with pytest.raises(AssertionError, match="1 of 8 elements differ"):
            LC.assert_same_bits(x, y, name)
    assert not LC.same_bits(x, x.reshape(4, 2))
    with pytest.raises(AssertionError):
        LC.assert_same_bits(x, x.astype(np.float64), "dtype")
