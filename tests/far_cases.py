"""Patterns, compact references, device operands and the case tables of the "far" tests: every
kernel run where 32-bit byte offsets and the packed 22-bit fields run out (no GPU here:
tests/test_far_cases_cpu.py checks this module; tests/test_gpu_far_sddmm.py, test_gpu_far_spmm.py
and test_gpu_far_attention.py use it).

A far pattern has few stored entries (under 10^4) whose row and column indices sit at the extremes
of a very large index space: only in short bands of consecutive indices (bands()): the first
indices, a band straddling every index whose byte offset is 2^31 or 2^32 (marks()) where the
operand goes that far, and the last indices. Inside band x band about `density` of the entries is
stored, so that column runs of several entries exist; a fully dense 16 x 16 block (a BSMR dense
tile) and a hub row or column longer than the SpMM / attention chunk are optional.

Full-size operands never exist on the host. A Far keeps the sorted used rows and columns and the
same pattern over them alone (`compact`: the entries keep their CSR order, since both maps are
monotone). The references are the suites' own (sddmm_cases.sddmm_ref, spmm_cases.spmm_ref,
attention_cases.selector_expected / attention_ref) on the compact pattern with compact operands from
the suites' own generators. On the device, device_operand() fills a tensor of the full shape with
NaN and writes the used rows alone: a stray read is a NaN or another finite value, never the right
one by luck.

fault_index() restates three address faults on the real indices: the unsigned and the signed
32-bit wrap of index x rowBytes, and a column field cut to 22 bits. gathered() / scattered() apply
one to a compact operand or result (a row outside the used set reads as NaN; a row nobody stores
stays NaN). tests/test_far_cases_cpu.py demands that every fault a case names changes its reference
result: a case that does not cross its boundary fails there, without a GPU.
"""
import collections
import functools

import numpy as np

import attention_cases as AC
import sddmm_cases as SD
import spmm_cases as SP
from bsmr import BF16, F16, F32

WIDTH = 32          # indices per band (merged bands stay within 64)
DENSITY = 0.3
MAX_ENTRIES = 10 ** 4
FAULTS = ("u32", "i32", "col22")

Far = collections.namedtuple("Far", "M N rowptr colidx rows cols compact")


def row_bytes(K, dtype):
    return K * (4 if dtype == F32 else 2)


def marks(rb, shift=0):
    """The row indices whose byte offset is 2^31 and 2^32 at rows of rb bytes (shift: every
    boundary scaled down by 2^shift, for the CPU self-check)."""
    return [(1 << 31 >> shift) // rb, (1 << 32 >> shift) // rb]


def bands(n, at=(), width=WIDTH):
    """[(start, length)] ascending and disjoint: the first `width` indices of [0, n), `width`
    indices around every mark of `at` that lies inside, the last `width`; overlapping bands merge."""
    spans = [(0, min(width, n)), (max(0, n - width), n)]
    spans += [(m - width // 2, m + width // 2) for m in at if m - width // 2 >= 0 and m + width // 2 <= n]
    out = []
    for a, b in sorted(spans):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b - a) for a, b in out]


def _band_indices(bs):
    return np.concatenate([np.arange(a, a + n, dtype=np.int64) for a, n in bs])


def far_pattern(M, N, row_bands, col_bands, density=DENSITY, seed=0, hub=None, block=None, cell=1):
    """Far of an M x N pattern, seeded and deterministic. Entries: about `density` of row band x
    column band; block = (row end, column end), each "first" or "last": a fully dense 16 x 16 block
    at that corner of the bands; hub = ("row" | "col", index, n): that row (column) holds n entries,
    the band columns (rows) first, then the lowest others; cell = 16: a block mask, whole 16 x 16
    cells of the bands stored or not."""
    rng = np.random.default_rng(seed)
    br, bc = _band_indices(row_bands), _band_indices(col_bands)
    assert br.max() < M and bc.max() < N
    keep = rng.random((-(-len(br) // cell), -(-len(bc) // cell))) < density
    keep = np.kron(keep, np.ones((cell, cell), bool))[:len(br), :len(bc)]
    r, c = [br[np.nonzero(keep)[0]]], [bc[np.nonzero(keep)[1]]]
    if block is not None:
        r0 = br[0] if block[0] == "first" else br[-1] - 15
        c0 = bc[0] if block[1] == "first" else bc[-1] - 15
        rr, cc = np.meshgrid(np.arange(r0, r0 + 16), np.arange(c0, c0 + 16), indexing="ij")
        r.append(rr.ravel())
        c.append(cc.ravel())
    if hub is not None:
        side, index, n = hub
        inband, size = (bc, N) if side == "row" else (br, M)
        assert n <= size and index < (M if side == "row" else N)
        others = np.setdiff1d(np.arange(min(size, 4096), dtype=np.int64), inband)
        line = np.concatenate([inband, others])[:n]
        assert len(line) == n
        fixed = np.full(n, index, np.int64)
        r.append(fixed if side == "row" else line)
        c.append(line if side == "row" else fixed)
    key = np.unique(np.concatenate(r) * np.int64(N) + np.concatenate(c))  # sorted by (row, column)
    r, c = key // N, key % N
    assert len(key) < MAX_ENTRIES, len(key)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=M))]).astype(np.uint32)
    rows, cols = np.unique(r), np.unique(c)
    rc = np.searchsorted(rows, r)
    rp_c = np.concatenate([[0], np.cumsum(np.bincount(rc, minlength=len(rows)))]).astype(np.uint32)
    compact = (len(rows), len(cols), rp_c, np.searchsorted(cols, c).astype(np.uint32))
    for a in (rowptr, rows, cols, compact[2], compact[3]):
        a.setflags(write=False)
    colidx = c.astype(np.uint32)
    colidx.setflags(write=False)
    return Far(int(M), int(N), rowptr, colidx, rows, cols, compact)


def full_pattern(far):
    return far.M, far.N, far.rowptr, far.colidx


def expand(Xc, used, n, fill=np.nan):
    """The full host array (n rows) of a compact one: the CPU self-check's small shapes only."""
    X = np.full((n,) + Xc.shape[1:], fill, Xc.dtype)
    X[used] = Xc
    return X


# ------------------------------------------------------------------------ address faults ----
def fault_index(idx, rb, fault):
    """The row a kernel would touch for row idx of an operand of rb-byte rows under `fault`: "u32":
    idx rb wraps at 2^32; "i32": the same offset read as signed (a negative row lies outside the
    allocation); "col22": idx cut to its low 22 bits."""
    idx = np.asarray(idx, np.int64)
    assert fault in FAULTS and (1 << 32) % rb == 0
    if fault == "col22":
        return idx & ((1 << 22) - 1)
    off = (idx * rb) % (1 << 32)
    if fault == "i32":
        off = np.where(off >= 1 << 31, off - (1 << 32), off)
    return off // rb


def _landing(used, rb, fault):
    f = fault_index(used, rb, fault)
    pos = np.clip(np.searchsorted(used, f), 0, len(used) - 1)
    return pos, used[pos] == f


def gathered(Xc, used, rb, fault):
    """The compact operand as a kernel with `fault` in its row address reads it: row i holds the
    row it lands on, NaN outside the used set (the device tensor's fill)."""
    pos, ok = _landing(used, rb, fault)
    return np.where(ok[:, None], Xc[pos], np.nan).astype(Xc.dtype)


def scattered(Yc, used, rb, fault):
    """The compact result as a kernel with `fault` in its store address leaves it: row i's values
    go where it lands; a row nobody stores keeps the NaN it started with."""
    pos, ok = _landing(used, rb, fault)
    out = np.full(Yc.shape, np.nan, Yc.dtype)
    out[pos[ok]] = Yc[ok]
    return out


def differs(a, b):
    """Bitwise: any element of a and b differs (NaN against a number differs)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return bool((a.view(np.uint64) != b.view(np.uint64)).any())


# ------------------------------------------------------------------------------ SDDMM ----
# runs: (K, dtype) the case launches; faults: (operand "A" | "B", fault) every run must catch, at
# that run's row bytes; at: the row bytes whose 2^31 / 2^32 marks place the bands
SddmmCase = collections.namedtuple("SddmmCase", "name M N runs at block faults hub density col_marks",
                                    defaults=(None, DENSITY, ()))


def _sddmm_cases():
    h21, h22 = 1 << 21, 1 << 22
    c = [
        SddmmCase("rb_B_below_4G", 96, h21 - 1, [(512, F32)], 2048, ("last", "last"), [("B", "i32")]),
        SddmmCase("rb_B_1k", 96, h22 - 1, [(512, BF16), (256, F32)], 1024, None, [("B", "i32")]),
        # a piece word of all ones needs 16 entries of column 2^22 - 1 inside one item, and the
        # scheduler deals a plan's entries to some 500 items whatever its size (measured: runs of 6 at
        # 1,300 entries, of 15 at 6,200 entries three quarters full). So this one case is full inside
        # its bands, three column bands wide (64 rows x 96 columns = 6,144 entries, every column a
        # run of 32 per row band), and the launch is asked for (layout rowblock: full tiles make the
        # plan tile-dominated)
        SddmmCase("rb_col_all_ones", 96, h22, [(128, F32), (256, F16)], 512, None, [], None, 1.0, (h21,)),
        SddmmCase("cm_B_at_4G", 96, h21, [(512, F32)], 2048, None, [("B", "i32")]),
        SddmmCase("cm_B_past_4G", 96, h21 + 64, [(512, F32), (1024, F16)], 2048, ("last", "last"),
                  [("B", "u32"), ("B", "i32")]),
        SddmmCase("cm_N_past_2p22", 96, h22 + 1, [(16, F32), (32, BF16)], 64, None, [("B", "col22")]),
        SddmmCase("rb_A_past_4G", h21 + 64, 192, [(512, F32), (1024, BF16)], 2048, None,
                  [("A", "u32"), ("A", "i32")]),
        # col_blocks = 1 where it is legal: the swapped operand's offsets right up to the limit
        SddmmCase("cols_A_below_4G", h21 - 1, 192, [(512, F32)], 2048, None, [("A", "i32")]),
    ]
    return {x.name: x for x in c}


SDDMM_CASES = _sddmm_cases()


def sddmm_far_spec(case, shift=0):
    """far_pattern's arguments for an SddmmCase; shift > 0: the same band layout with M, N and every
    boundary scaled down by 2^shift (the small dimension stays)."""
    def dim(n):  # 2^p + d -> 2^(p - shift) + d
        p = 1 << int(round(np.log2(n)))
        return n if n < 4096 else (p >> shift) + (n - p)

    M, N = dim(case.M), dim(case.N)
    at = marks(case.at, shift)
    col_at = at + [m >> shift for m in case.col_marks]
    return dict(M=M, N=N, row_bands=bands(M, at), col_bands=bands(N, col_at), density=case.density,
                seed=sum(case.name.encode()), block=case.block,
                hub=case.hub and (case.hub[0], (M if case.hub[0] == "row" else N) - 1, case.hub[2]))


@functools.lru_cache(maxsize=None)
def sddmm_far(name):
    return far_pattern(**sddmm_far_spec(SDDMM_CASES[name]))


@functools.lru_cache(maxsize=8)
def sddmm_reference(far_key, K, dtype, data):
    """(Ac, Bc, P, S): compact operands as the kernel sees them and the float64 reference;
    far_key: an SDDMM_CASES name."""
    far = sddmm_far(far_key)
    return compact_sddmm(far, K, dtype, data)


def compact_sddmm(far, K, dtype, data, seed=0):
    gen = {"grid": SD.grid_data, "signed": SD.signed_data}[data]
    Mc, Nc = far.compact[0], far.compact[1]
    Ac = SD.as_seen(gen(Mc * K, 101 + 2 * seed), dtype).reshape(Mc, K)
    Bc = SD.as_seen(gen(Nc * K, 202 + 2 * seed), dtype).reshape(Nc, K)
    P, S = SD.sddmm_ref(far.compact, Ac, Bc)
    return Ac, Bc, P, S


def sddmm_faulted(far, Ac, Bc, operand, rb, fault):
    """The reference result under one address fault in the gather of `operand`."""
    with np.errstate(invalid="ignore"):
        if operand == "A":
            return SD.sddmm_ref(far.compact, gathered(Ac, far.rows, rb, fault), Bc)[0]
        return SD.sddmm_ref(far.compact, Ac, gathered(Bc, far.cols, rb, fault))[0]


@functools.lru_cache(maxsize=None)
def half_launch_far(kind):
    """128 x (2^21 + 128) for the two remaining fp16 / bf16 launches at bf16 K 512 (1 KiB rows: B
    passes 2 GiB): "dense": the usual bands, run with dense_min lowered until the dense-sampled
    launch is chosen; "ptile": a 16 x 16 block mask over the same bands, run with ptile = 1."""
    N = (1 << 21) + 128
    return far_pattern(128, N, bands(128), bands(N, marks(1024)), seed=51 if kind == "dense" else 52,
                       density=DENSITY if kind == "dense" else 0.5, cell=1 if kind == "dense" else 16)


# ------------------------------------------------------------------------------- SpMM ----
SPMM_CHUNK = 32
# runs: (side, K, dtype); faults per run: (array "X" | "Y", fault) at 2 KiB rows (K 512 fp32 X and
# Y rows, K 1024 bf16 X rows)
SPMM_RUNS = {
    "bigN": [(1, 512, F32, [("X", "u32"), ("X", "i32")]), (2, 512, F32, [("Y", "u32"), ("Y", "i32")]),
             (1, 1024, BF16, [("X", "u32"), ("X", "i32")])],
    "bigM": [(1, 512, F32, [("Y", "u32"), ("Y", "i32")]), (2, 512, F32, [("X", "u32"), ("X", "i32")]),
             (2, 1024, BF16, [("X", "u32"), ("X", "i32")])],
}


@functools.lru_cache(maxsize=None)
def spmm_far(name):
    """bigN: 96 x (2^21 + 64), the last column a hub of all 96 rows; bigM: (2^21 + 64) x 192, the
    last row a hub of all 192 columns. With chunk 32 the hubs and the band rows (about 38 entries)
    are split destinations."""
    big = (1 << 21) + 64
    if name == "bigN":
        return far_pattern(96, big, bands(96), bands(big, marks(2048)), seed=31, hub=("col", big - 1, 96))
    if name == "bigM":
        return far_pattern(big, 192, bands(big, marks(2048)), bands(192), seed=32, hub=("row", big - 1, 192))
    raise KeyError(name)


def spmm_used(far, side):
    """(destinations used, sources used, destinations of the full shape, sources)."""
    return (far.rows, far.cols, far.M, far.N) if side == 1 else (far.cols, far.rows, far.N, far.M)


def compact_spmm(far, side, K, dtype, data, seed=0):
    """(V, Xc, ref): values (nnz), compact X as the kernel sees it, spmm_ref on the compact pattern."""
    nnz = len(far.colidx)
    ns = len(spmm_used(far, side)[1])
    if data == "grid":
        V, X = SP.grid_values(nnz, 7 + seed), SD.grid_data(ns * K, 8 + seed)
    else:
        V, X = SP.signed_values(nnz, 7 + seed), SD.signed_data(ns * K, 8 + seed)
    Xc = SD.as_seen(X, dtype).reshape(ns, K)
    return V, Xc, SP.spmm_ref(far.compact, side, V, Xc)


def spmm_faulted(far, side, V, Xc, ref, array, rb, fault):
    dst, src, _, _ = spmm_used(far, side)
    with np.errstate(invalid="ignore"):
        if array == "X":
            return SP.spmm_ref(far.compact, side, V, gathered(Xc, src, rb, fault))[0]
    return scattered(ref[0], dst, rb, fault)


# -------------------------------------------------------------------------- attention ----
# runs: (D, Dv, dtype, faults): (array "Q" | "K" | "V" | "O", fault), at the array's own row bytes
ATTN_RUNS = {
    "bigN": [(256, 256, F32, [("K", "u32"), ("K", "i32"), ("V", "u32"), ("V", "i32")]),
             (512, 256, BF16, [("K", "u32"), ("K", "i32"), ("V", "i32")])],
    "bigM": [(256, 256, F32, [("Q", "u32"), ("Q", "i32"), ("O", "u32"), ("O", "i32")])],
}


@functools.lru_cache(maxsize=None)
def attention_far(name):
    """bigN: 96 x (2^22 + 64): K and V of 1 KiB rows are 4 GiB each; bigM: (2^22 + 64) x 320, Q
    and O 4 GiB each, the last row a hub of 300 entries (a split row: scratch, the reduce kernel
    and the far end of O)."""
    big = (1 << 22) + 64
    if name == "bigN":
        return far_pattern(96, big, bands(96), bands(big, marks(1024)), seed=41)
    if name == "bigM":
        return far_pattern(big, 320, bands(big, marks(1024)), bands(320), seed=42, hub=("row", big - 1, 300))
    raise KeyError(name)


def attention_faulted(far, Q, K, V, scale, dtype, array, fault):
    """(O, LSE) float64 of attention_ref under one address fault."""
    D, Dv = Q.shape[1], V.shape[1]
    esz = 4 if dtype == F32 else 2
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if array == "Q":
            Q = gathered(SD.as_seen(Q, dtype), far.rows, D * esz, fault)
        elif array == "K":
            K = gathered(SD.as_seen(K, dtype), far.cols, D * esz, fault)
        elif array == "V":
            V = gathered(SD.as_seen(V, dtype), far.cols, Dv * esz, fault)
        ref = AC.attention_ref(far.compact, Q, K, V, scale, dtype)
    if array == "O":
        return scattered(ref["O"], far.rows, Dv * 4, fault), ref["LSE"]
    return ref["O"], ref["LSE"]


# ------------------------------------------------------- device helpers (GPU tests only) ----
def device_operand(n, used, Xc, dtype):
    """A device tensor of the full shape (n x Xc.shape[1], of `dtype`) filled with NaN, the used
    rows written from the compact host array, which is converted on the host as
    gpu_util.to_device does."""
    from gpu_util import torch_cuda, torch_dtype
    torch = torch_cuda()
    tdt = torch_dtype(dtype)
    X = torch.full((int(n), Xc.shape[1]), float("nan"), dtype=tdt, device="cuda")
    X.index_copy_(0, torch.from_numpy(np.array(used, np.int64)).cuda(),
                  torch.from_numpy(np.array(Xc, np.float32)).to(tdt).cuda())
    return X


def take_rows(dY, used):
    """(the used rows on the host, numpy; the number of non-zero elements in every other row). The
    used rows are zeroed in place for the count: nothing of the full size is copied or returned."""
    from gpu_util import torch_cuda
    torch = torch_cuda()
    idx = torch.from_numpy(np.array(used, np.int64)).cuda()
    got = dY.index_select(0, idx).cpu().numpy()
    dY.index_fill_(0, idx, 0)
    return got, int(torch.count_nonzero(dY))
