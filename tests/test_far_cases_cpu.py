"""CPU: the far tests' checker is checked (tests/far_cases.py).

  * the generator: bands of 32 to 64 indices at the first indices, around every 2^31 / 2^32 byte
    mark the operand reaches and at the last indices; deterministic; under 10^4 entries; the
    compact pattern keeps the CSR order;
  * (a) every SDDMM case with the same band layout and every boundary scaled down by 2^11 (2^21
    becomes 2^10): full operands are built and the compact reference equals sddmm_ref on the full
    arrays bit for bit; the same for one SpMM and one attention shape;
  * (b) every GPU case, on its real indices, under the address faults it names (unsigned and
    signed 32-bit wrap of index x rowBytes, a column cut to 22 bits): each must change the reference
    result bitwise. A case that does not cross its boundary fails here.
"""
import numpy as np
import pytest

import attention_cases as AC
import far_cases as FC
import sddmm_cases as SD
import spmm_cases as SP
from bsmr import BF16, F16, F32

SHIFT = 11


def test_fault_index_restates_the_three_faults():
    h21 = 1 << 21
    idx = np.array([0, 5, h21 - 1, h21, h21 + 63, (1 << 20), (1 << 22) - 1, 1 << 22, (1 << 22) + 64])
    assert FC.fault_index(idx, 2048, "u32").tolist() == [0, 5, h21 - 1, 0, 63, 1 << 20, h21 - 1, 0, 64]
    assert FC.fault_index(idx, 2048, "i32").tolist() == [0, 5, -1, 0, 63, -(1 << 20), -1, 0, 64]
    assert FC.fault_index(idx, 64, "u32").tolist() == idx.tolist()  # 64-byte rows: no wrap below 2^26
    assert FC.fault_index(idx, 64, "col22").tolist() == [0, 5, h21 - 1, h21, h21 + 63, 1 << 20, (1 << 22) - 1, 0, 64]
    used = np.array([0, 1, 63, h21 + 63])
    X = np.arange(8, dtype=np.float32).reshape(4, 2)
    g = FC.gathered(X, used, 2048, "u32")
    assert np.array_equal(g[:3], X[:3]) and np.array_equal(g[3], X[2])  # row 2^21 + 63 reads row 63
    g = FC.gathered(X, np.array([0, 1, 63, h21 + 62]), 2048, "u32")
    assert np.isnan(g[3]).all()  # row 62 is not a used row: the device tensor's NaN
    s = FC.scattered(X, used, 2048, "u32")
    assert np.array_equal(s[2], X[3]) and np.isnan(s[3]).all() and np.array_equal(s[:2], X[:2])


def test_bands():
    assert FC.bands(96) == [(0, 32), (64, 32)]
    assert FC.bands(40) == [(0, 40)]
    n = (1 << 21) + 64
    assert FC.bands(n, FC.marks(2048)) == [(0, 32), ((1 << 20) - 16, 32), ((1 << 21) - 16, 32), (n - 32, 32)]
    assert FC.bands((1 << 21) - 1, FC.marks(2048)) == [(0, 32), ((1 << 20) - 16, 32), ((1 << 21) - 33, 32)]
    assert FC.bands(1 << 21, FC.marks(2048)) == [(0, 32), ((1 << 20) - 16, 32), ((1 << 21) - 32, 32)]
    assert FC.bands((1 << 21) + 20, FC.marks(2048))[-1] == ((1 << 21) - 16, 36)  # merged


def _all_fars():
    out = [("sddmm/" + n, lambda n=n: FC.sddmm_far(n)) for n in FC.SDDMM_CASES]
    out += [("spmm/" + n, lambda n=n: FC.spmm_far(n)) for n in FC.SPMM_RUNS]
    out += [("attention/" + n, lambda n=n: FC.attention_far(n)) for n in FC.ATTN_RUNS]
    return out


@pytest.mark.parametrize("name,make", _all_fars(), ids=[n for n, _ in _all_fars()])
def test_far_pattern_shape(name, make):
    far = make()
    M, N, rp, ci = FC.full_pattern(far)
    nnz = len(ci)
    assert 0 < nnz < FC.MAX_ENTRIES and rp[0] == 0 and rp[-1] == nnz and len(rp) == M + 1
    assert rp.dtype == np.uint32 and ci.dtype == np.uint32
    rows = SP.entry_rows(M, rp)
    key = rows * N + ci.astype(np.int64)
    assert (np.diff(key) > 0).all()  # sorted rows, no duplicate
    assert np.array_equal(np.unique(rows), far.rows) and np.array_equal(np.unique(ci), far.cols)
    # the extremes are used, and the compact pattern is the same entries in the same order
    assert far.rows[0] == 0 and far.rows[-1] == M - 1 and far.cols[0] == 0 and far.cols[-1] == N - 1
    Mc, Nc, rpc, cic = far.compact
    assert (Mc, Nc) == (len(far.rows), len(far.cols))
    assert np.array_equal(far.rows[SP.entry_rows(Mc, rpc)], rows) and np.array_equal(far.cols[cic], ci)
    # indices come from bands of 32 .. 64 consecutive indices (a hub adds the lowest others)
    for used, hub in ((far.rows, name == "spmm/bigN"), (far.cols, "bigM" in name)):
        runs = np.split(used, np.nonzero(np.diff(used) != 1)[0] + 1)
        assert all(len(r) <= 64 for r in runs) or hub, [len(r) for r in runs]
        assert len(used) <= 400
    # column runs of several entries exist
    assert np.bincount(cic).max() >= 4


def test_far_pattern_is_seeded():
    a = FC.far_pattern(96, 5000, FC.bands(96), FC.bands(5000, [2048]), seed=3, block=("last", "last"))
    b = FC.far_pattern(96, 5000, FC.bands(96), FC.bands(5000, [2048]), seed=3, block=("last", "last"))
    c = FC.far_pattern(96, 5000, FC.bands(96), FC.bands(5000, [2048]), seed=4, block=("last", "last"))
    assert np.array_equal(a.colidx, b.colidx) and np.array_equal(a.rowptr, b.rowptr)
    assert not np.array_equal(a.colidx, c.colidx)
    # the dense block: the last 16 rows hold each of the last 16 columns
    M, N, rp, ci = FC.full_pattern(a)
    for r in range(80, 96):
        assert set(range(N - 16, N)) <= set(ci[rp[r]:rp[r + 1]].tolist())
    h = FC.far_pattern(5000, 320, FC.bands(5000), FC.bands(320), seed=1, hub=("row", 4999, 300))
    assert h.rowptr[5000] - h.rowptr[4999] == 300 and h.compact[1] >= 300


# ---- (a) compact reference == the reference on full arrays, every boundary scaled down by 2^11 ----
@pytest.mark.parametrize("name", sorted(FC.SDDMM_CASES))
def test_compact_reference_equals_full_reference_scaled(name):
    case = FC.SDDMM_CASES[name]
    spec = FC.sddmm_far_spec(case, SHIFT)
    real = FC.sddmm_far_spec(case)
    assert len(spec["row_bands"]) == len(real["row_bands"]) and len(spec["col_bands"]) == len(real["col_bands"])
    assert max(spec["M"], spec["N"]) <= (1 << 11) + 64
    far = FC.far_pattern(**spec)
    for K, dtype in case.runs:
        K = min(K, 64)
        Ac, Bc, P, S = FC.compact_sddmm(far, K, dtype, "signed")
        A, B = FC.expand(Ac, far.rows, far.M), FC.expand(Bc, far.cols, far.N)
        Pf, Sf = SD.sddmm_ref(FC.full_pattern(far), A, B)
        assert np.isfinite(Pf).all() and not FC.differs(P, Pf) and not FC.differs(S, Sf)


def test_compact_spmm_and_attention_equal_full_scaled():
    n = (1 << 10) + 64
    far = FC.far_pattern(96, n, FC.bands(96), FC.bands(n, [512, 1024]), seed=5, hub=("col", n - 1, 96))
    for side in (1, 2):
        V, Xc, ref = FC.compact_spmm(far, side, 32, F32, "signed")
        dst, src, nd, ns = FC.spmm_used(far, side)
        Y, S, cnt = SP.spmm_ref(FC.full_pattern(far), side, V, FC.expand(Xc, src, ns, fill=0.0))
        assert not FC.differs(Y[dst], ref[0]) and not FC.differs(S[dst], ref[1])
        assert np.array_equal(cnt[dst], ref[2])
        rest = np.ones(nd, bool)
        rest[dst] = False
        assert (Y[rest] == 0).all() and (cnt[rest] == 0).all()
    far = FC.far_pattern(n, 320, FC.bands(n, [512, 1024]), FC.bands(320), seed=6, hub=("row", n - 1, 300))
    Q, K, V, opscale = AC.signed_inputs(far.compact, 32, 48, "narrow", 0.125)
    ref = AC.attention_ref(far.compact, Q, K, V, 0.125)
    full = AC.attention_ref(FC.full_pattern(far), FC.expand(Q, far.rows, far.M, 0.0), FC.expand(K, far.cols, far.N, 0.0),
                            FC.expand(V, far.cols, far.N, 0.0), 0.125)
    assert not FC.differs(full["O"][far.rows], ref["O"]) and not FC.differs(full["LSE"][far.rows], ref["LSE"])
    rest = np.ones(far.M, bool)
    rest[far.rows] = False
    assert (full["O"][rest] == 0).all() and (full["LSE"][rest] == -np.inf).all()


# ---- (b) every GPU case under the address faults it names, on its real indices ----------------------
@pytest.mark.parametrize("name", sorted(FC.SDDMM_CASES))
def test_sddmm_cases_cross_their_boundaries(name):
    case = FC.SDDMM_CASES[name]
    far = FC.sddmm_far(name)
    for K, dtype in case.runs:
        Ac, Bc, P, _ = FC.sddmm_reference(name, K, dtype, "grid")
        assert np.isfinite(P).all()
        assert not FC.differs(P, SD.sddmm_ref(far.compact, Ac, Bc)[0])
        for operand, fault in case.faults:
            Pf = FC.sddmm_faulted(far, Ac, Bc, operand, FC.row_bytes(K, dtype), fault)
            assert FC.differs(P, Pf), f"{name} K {K}: a {fault} fault on {operand} goes unseen"
    # the faults a case does not name because its shape stays inside: they must indeed change nothing
    inside = {"rb_B_below_4G": [("B", "u32")], "rb_B_1k": [("B", "u32")], "rb_col_all_ones": [("B", "u32"), ("B", "i32")],
              "cm_B_at_4G": [("B", "u32")], "cols_A_below_4G": [("A", "u32")]}
    K, dtype = case.runs[0]
    Ac, Bc, P, _ = FC.sddmm_reference(name, K, dtype, "grid")
    for operand, fault in inside.get(name, []):
        assert not FC.differs(P, FC.sddmm_faulted(far, Ac, Bc, operand, FC.row_bytes(K, dtype), fault))


def test_half_launch_patterns_cross_2_GiB():
    for kind in ("dense", "ptile"):
        far = FC.half_launch_far(kind)
        Ac, Bc, P, _ = FC.compact_sddmm(far, 512, BF16, "grid")
        assert FC.differs(P, FC.sddmm_faulted(far, Ac, Bc, "B", 1024, "i32")), kind
    M, N, rp, ci = FC.full_pattern(FC.half_launch_far("ptile"))
    assert len(ci) % 256 == 0 and (np.diff(rp.astype(np.int64))[:16] == np.diff(rp.astype(np.int64))[0]).all()


def test_sddmm_case_shapes():
    """The shapes of the issue's table, and what each is there for."""
    h21, h22 = 1 << 21, 1 << 22
    shape = {n: (c.M, c.N) for n, c in FC.SDDMM_CASES.items()}
    assert shape == {"rb_B_below_4G": (96, h21 - 1), "rb_B_1k": (96, h22 - 1), "rb_col_all_ones": (96, h22),
                     "cm_B_at_4G": (96, h21), "cm_B_past_4G": (96, h21 + 64), "cm_N_past_2p22": (96, h22 + 1),
                     "rb_A_past_4G": (h21 + 64, 192), "cols_A_below_4G": (h21 - 1, 192)}
    # rb_col_all_ones: column 2^22 - 1 holds every used row
    far = FC.sddmm_far("rb_col_all_ones")
    M, N, rp, ci = FC.full_pattern(far)
    assert np.array_equal(SP.entry_rows(M, rp)[ci == h22 - 1], far.rows) and len(ci) == 64 * 96
    # rb_B_1k: column 2^22 - 2, the last, is used
    assert FC.sddmm_far("rb_B_1k").cols[-1] == h22 - 2
    # cm_N_past_2p22: column 2^22 is used, and so is column 0 it would be cut to
    assert FC.sddmm_far("cm_N_past_2p22").cols[-1] == h22 and FC.sddmm_far("cm_N_past_2p22").cols[0] == 0


@pytest.mark.parametrize("name", sorted(FC.SPMM_RUNS))
def test_spmm_cases_cross_their_boundaries(name):
    far = FC.spmm_far(name)
    lens = {side: SP.list_lengths(far.compact, side) for side in (1, 2)}
    assert lens[1].max() > FC.SPMM_CHUNK and lens[2].max() > FC.SPMM_CHUNK  # split destinations on both sides
    for side, K, dtype, faults in FC.SPMM_RUNS[name]:
        V, Xc, ref = FC.compact_spmm(far, side, K, dtype, "grid")
        for array, fault in faults:
            rb = FC.row_bytes(K, dtype) if array == "X" else 4 * K
            Yf = FC.spmm_faulted(far, side, V, Xc, ref, array, rb, fault)
            assert FC.differs(ref[0], Yf), f"{name} side {side} K {K}: a {fault} fault on {array} goes unseen"
    # the hub is a far destination and longer than the chunk
    hub = lens[2][-1] if name == "bigN" else lens[1][-1]
    assert hub == (96 if name == "bigN" else 192)


@pytest.mark.parametrize("name", sorted(FC.ATTN_RUNS))
def test_attention_cases_cross_their_boundaries(name):
    far = FC.attention_far(name)
    chunk = AC.limits()["chunk"]
    if name == "bigM":
        assert AC.row_lengths(far.compact)[-1] == 300 > chunk  # the last row is split
    for D, Dv, dtype, faults in FC.ATTN_RUNS[name]:
        Q, K, V, winner, pi, base = AC.selector(far.compact, D, Dv, "random", dtype)
        ref = AC.attention_ref(far.compact, Q, K, V, 0.125, dtype)
        O, LSE = AC.selector_expected(V, winner, pi, base, 0.125, dtype)
        assert not FC.differs(ref["O"], O) and not FC.differs(ref["LSE"], LSE)  # the exact data's own claim
        for array, fault in faults:
            Of, Lf = FC.attention_faulted(far, Q, K, V, 0.125, dtype, array, fault)
            assert FC.differs(ref["O"], Of) or FC.differs(ref["LSE"], Lf), \
                f"{name} D {D} {AC.DTYPE_NAME[dtype]}: a {fault} fault on {array} goes unseen"
