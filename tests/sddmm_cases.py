"""float64 reference, data sets, error bound and the launch-path table of the forward SDDMM tests
(no GPU here: tests/test_sddmm_ref_cpu.py checks this module, tests/test_gpu_sddmm_float64.py and
tests/test_gpu_sddmm_edges.py use it).

Reference: sddmm_ref, numpy float64 straight from the CSR on the operands as the kernel sees them
(fp16 / bf16 rounded on the host by gpu_util.half_values): P = sum_k a b and S = sum_k |a b| per
stored entry. It calls neither the library nor the oracle.

Data:
  * grid_data: integer multiples of 1/8 in [-4, 4) (6 significant bits: exact in fp32, fp16 and
    bf16). Every product is a multiple of 2^-6 of magnitude <= 16, so every partial sum of up to
    2048 products, in any order, is a multiple of 2^-6 below 2^15: at most 21 bits. The fp32 result
    is therefore exact whatever the summation order, tile shape or lane split, and the tests demand
    P == ref bit for bit: a dropped, doubled or misplaced term, a wrong row, a narrowed accumulator
    or store all fail with no tolerance.
  * signed_data: uniform [-1, 1) in fp32 (full mantissa), held to sddmm_bound.
  * identity_data (patterns with M, N <= 4096, any K >= 16): operands that make stored entry
    (i, j) equal 4096 i + j. Six columns pos[t] = t K // 6 carry everything, the rest is zero:
    A[i, pos[k]] = digit_k(i) 16^k against B[j, pos[k]] = 4096, and A[i, pos[3 + k]] = 16^k against
    B[j, pos[3 + k]] = digit_k(j) (base-16 digits, k = 0, 1, 2). Every operand has at most four
    significant bits and magnitude <= 4096 (exact in fp16 and bf16), every product and every
    partial sum in any order is an integer below 2^24 (exact in fp32). Every entry of a pattern
    has its own value, so under assert_exact a misplaced, swapped, missing or doubled store fails
    with certainty and names the entry; grid data catches a misplaced value only when the two
    entries' values differ (tests/test_store_ref_cpu.py measures how often they do not).

Bound: |P - ref| <= min(2 K, 8 sqrt K) 2^-24 S + 1e-6 scale.
  * 2 K 2^-24 S is the deterministic bound of a K-term fp32 sum of once-rounded products
    (spmm_cases.signed_bound; the fp32 MFMA is a k-ordered fmaf chain, and a product of two halves
    is exact in fp32).
  * 8 sqrt(K) 2^-24 S is the Higham-Mary probabilistic bound with lambda = 8 (a false failure per
    element has probability about 2 exp(-32)); it is the tighter one from K = 16 on.
  * `scale` is the product of the two operands' scalings (1 for plain data): the absolute term
    covers entries whose S is tiny.
  The bound is derived, never widened from what a GPU shows; each GPU test prints its worst
  error / bound ratio (DESIGN.md §11.1 records them).

CASES: one entry per kernel instantiation the dispatch can reach (csrc/launch_select.cpp
choose_launch, rb_form; csrc/sddmm.hip pick_kernel / pick_k, launch_rb; csrc/rb_kernel.hpp pick_rb;
csrc/sddmm_half.hip launch_half, launch_ptile; csrc/sddmm_dense.hip launch_dense), on the smallest
pattern of the suite that takes it, with the plan options that select the path, the Plan.stats()
evidence that it ran and the library's own account of the launch (check_stats):

  column-major fp32 (k_sddmm_f32<KT, G>; `colmajor`: no lazily built layout exists afterwards)
    G = 4, generic KT: K = 16, 48       G = 8, generic: K = 96       G = 8, KT = 32: K = 32
    G = 16, fixed KT: K = 64, 128, 256, 512          G = 16, generic: K = 192, 1024
    a residual-only pattern (`empty`: no dense tile) and `blocky` (tiles only, the auto rule)
  column-major fp16 / bf16 (k_sddmm_half<BF16>): K = 32, 96 (auto), 128, 512 (layout colmajor),
    and `blocky` with ptile = 0 (tile-dominated: the auto rule keeps the column-major tile launch)
  row-block (k_sddmm_rb / k_sddmm_rb_pair<DT, RBY, NT, DYN, LITE>; rb_items[slot] > 0):
    fp32 K = 32 .. 512 and fp16 / bf16 K = 64 .. 1024 (rows of 128 B .. 2 KiB, both half types at
    512 B and 2 KiB); the forms at 512-byte rows, fp32 K = 128 and bf16 K = 256: lite default,
    out_staged = 1, out_staged = 1 with pair_min_items = 0 (rb_pairs; also at 2 KiB rows, the
    pair kernel without batches), batches = 1 (rb_batches; alone, staged, and paired),
    orig_rows = 1 (rb_orig_rows), col_blocks = 1 (rb_col_blocks), tile_min_f32 / tile_min_half = 0
    (rb_tiles: kept tiles on MFMA), l2_range_kb = 64, rb_rows = 16 (rb_rows[slot] == 16),
    out_packed = 0; and pick_rb's whole product (`rbx_*`): every dtype and row size at 512 and 1024
    threads per workgroup (rb_rows = 16, or an A image past 80 KiB; the geometry's thread count is
    checked), lite and full (staged output), fixed phases and dynamic batches (rows <= 512 B), the
    pair kernel (rows >= 512 B; with batches at 512 B), without kept tiles
  dense-sampled (k_sddmm_dense<DT, 64, NS, NW>; dense_sampled_tiles > 0): uniform_mask(300, 0.2)
    (M and N no multiple of the 128-wide tile), both dtypes: K = 64 (one chunk) and 320 (five),
    dense_ks = 1 (four waves; the default at under 512 tiles is eight), dense_ns in {3, 4, 5}
  panel-tile (k_sddmm_ptile<BF16, NK, W>; ptile_items against the item list of the plan's
    blockOffsets): both dtypes at K = 64, 128, 256, 512 with ptile_tpi = 3 (four waves), 8 (eight
    waves, all busy), 64 on block_mask(768, 16, 0.2) (up to 17 tiles per item: more than waves) and
    the default equal runs (one tile each on block_mask(512, 16, 0.15); on the larger mask runs of
    two tiles, some over two panels); ptile = 1 on `zipf` (tiles and a residual in one launch)

The launch kind and, for a row-block launch, the kernel form (lite or full, single or pair, fixed
phases or dynamic batches, threads per workgroup) are read from the library (the debug export
bsmr_debug_plan_launch: the choose_launch and rb_form the launch itself goes through) and held to
what the case names: the `rbx_lite_*` / `rbx_full_*` / `rbx_pair_*` cases by their names, every
row-block case by the documented lite rule (no kept tile, direct stores, default staging). Not told
apart by any evidence the library exposes: the panel-tile workgroup size (it follows from
ptile_tpi). k_sddmm_dense's NS at four waves is always 2.

bsmr_sddmm_panels reaches the row-block kernels (a range's own layout) and, for fp32 without a
row-block slot, k_sddmm_panels_f32<KT, G>; sddmm_half.hip and sddmm_dense.hip have no panels
form (PANEL_CASES). Patterns: spmm_cases.pattern `zipf` (517 x 4000, 31,170 entries, M % 16 != 0,
71 dense tiles and a residual), `empty` (empty rows and columns, no dense tile), `hub` (one full
row), test_gpu_parity's `blocky`, the masks above, and `tall` (903 non-empty rows, 12,652
entries: enough rows for a 128-byte-row image past 80 KiB).
"""
import collections
import functools

import numpy as np

from bsmr import BF16, F16, F32, synth
from gpu_util import half_values
from spmm_cases import entry_rows, shuffled
from spmm_cases import pattern as _spmm_pattern

FREE = 288 * 1024 ** 3
DTYPE_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(M, N, rowptr, colidx), built once per process; callers do not modify the arrays."""
    if name in ("zipf", "empty", "hub", "zipf_shuffled"):
        return _spmm_pattern(name)
    if name == "band":  # 4096 x 4096, 215,552 entries: store_cases' large items (band_scatter)
        return band_scatter(4096, 4096, 64, 1100, 36, seed=1)
    if name == "band_shuffled":  # the same with every row's columns in random order
        return shuffled(pattern("band"))
    if name == "blocky":  # test_gpu_parity.small_cases()["blocky"]: 147 full tiles, no residual
        return synth.block_mask(512, 16, 0.15, seed=4)
    if name == "blockmask":  # test_gpu_ptile's mask: 164 full tiles, 16 empty rows
        return synth.block_mask(512, 16, 0.15, seed=11)
    if name == "blockmask768":  # test_gpu_ptile's larger mask: 459 full tiles (more than CUs), up to 17
        return synth.block_mask(768, 16, 0.2, seed=12)  # per panel (more than waves); 117,504 entries
    if name == "tall":  # 903 non-empty rows (over 640: a 128-byte-row image past 80 KiB), 12,652 entries
        return synth.random_rows(1000, 600, 14, seed=9, zipf=1.1, empty_frac=0.1)
    if name == "uniform300":  # 19 % dense, 3 x 3 tiles of 128 with ragged last tiles
        return synth.uniform_mask(300, 0.2, 7)
    raise KeyError(name)


def band_scatter(M, N, band_rows, band_cols, per_row, seed):
    """Rows [0, band_rows) hold the columns [0, band_cols) and nothing else (a dense band: column
    runs of 16 in every row block, long runs of consecutive CSR positions); every other row holds
    per_row columns drawn at random (single-entry column runs). Rows are column-sorted."""
    rng = np.random.default_rng(seed)
    cols = [np.arange(band_cols) if r < band_rows else np.sort(rng.choice(N, per_row, replace=False))
            for r in range(M)]
    rp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.uint32)
    return M, N, rp, np.concatenate(cols).astype(np.uint32)


def as_seen(X, dtype):
    """X (fp32) as the kernel sees it: rounded to fp16 / bf16 for the half dtypes."""
    X = np.ascontiguousarray(X, np.float32)
    return X if dtype == F32 else half_values(X, dtype)


def sddmm_ref(pat, A, B, dtype=F32):
    """float64 (P, S) per stored entry, CSR order: P = sum_k a b, S = sum_k |a b|, on A (M x K) and
    B (N x K) rounded to `dtype` first. Blocks of entries keep the temporaries near 100 MB."""
    M, N, rp, ci = pat
    nnz = len(ci)
    A = as_seen(A, dtype).reshape(M, -1)
    B = as_seen(B, dtype).reshape(N, -1)
    K = A.shape[1]
    assert B.shape[1] == K
    rows = entry_rows(M, rp)
    cols = np.asarray(ci, np.int64)
    P = np.empty(nnz, np.float64)
    S = np.empty(nnz, np.float64)
    step = max(1, (3 << 20) // K)
    with np.errstate(invalid="ignore", over="ignore"):  # non-finite operands propagate quietly
        for e0 in range(0, nnz, step):
            e1 = min(nnz, e0 + step)
            t = A[rows[e0:e1]].astype(np.float64)
            t *= B[cols[e0:e1]]
            P[e0:e1] = t.sum(axis=1)
            np.abs(t, out=t)
            S[e0:e1] = t.sum(axis=1)
    return P, S


def grid_data(n, seed):
    """n fp32 values k / 8, k integer in [-32, 32): exact in fp32, fp16 and bf16."""
    k = np.random.default_rng(seed).integers(-32, 32, int(n))
    return (k / 8.0).astype(np.float32)


def signed_data(n, seed):
    """n fp32 values uniform in [-1, 1) (full mantissa; the caller rounds for half dtypes)."""
    return np.random.default_rng(seed).random(int(n), dtype=np.float32) * np.float32(2) - np.float32(1)


def identity_data(M, N, K):
    """(A, B), fp32 M x K and N x K, with sum_k A[i, k] B[j, k] = 4096 i + j exactly in fp32, fp16
    and bf16 in any summation order (module docstring). M, N <= 4096, K >= 16."""
    assert M <= 4096 and N <= 4096 and K >= 16
    pos = [t * K // 6 for t in range(6)]
    A = np.zeros((M, K), np.float32)
    B = np.zeros((N, K), np.float32)
    i, j = np.arange(M), np.arange(N)
    for k in range(3):
        A[:, pos[k]] = ((i >> (4 * k)) & 15) * 16 ** k
        B[:, pos[k]] = 4096
        A[:, pos[3 + k]] = 16 ** k
        B[:, pos[3 + k]] = (j >> (4 * k)) & 15
    return A, B


def identity_values(pat):
    """What identity data makes of every stored entry: 4096 row + column (float64, CSR order)."""
    M, _, rp, ci = pat
    return 4096.0 * entry_rows(M, rp) + np.asarray(ci, np.float64)


def sddmm_bound(S, K, scale=1.0):
    """Per entry: min(2 K, 8 sqrt K) 2^-24 S + 1e-6 scale (module docstring)."""
    return min(2.0 * K, 8.0 * np.sqrt(K)) * 2.0 ** -24 * np.asarray(S, np.float64) + 1e-6 * scale


def bound_ratio(P, ref, S, K, scale=1.0):
    """max over entries of |P - ref| / bound (inf when an entry is not finite)."""
    err = np.abs(np.asarray(P, np.float64) - ref)
    r = err / sddmm_bound(S, K, scale)
    return float(np.where(np.isfinite(r), r, np.inf).max()) if len(r) else 0.0


def assert_exact(P, ref, what):
    """P (fp32) equals the exact float64 reference bit for bit, every entry written."""
    assert np.isfinite(P).all(), f"{what}: {int((~np.isfinite(P)).sum())} entries never written"
    bad = np.nonzero(P.astype(np.float64) != ref)[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(P)} entries differ from the exact result, first "
                           f"{bad[:5]}: got {P[bad[:5]]} want {ref[bad[:5]]}")


def assert_bound(P, ref, S, K, what, kind, scale=1.0):
    """P within sddmm_bound of the reference, every entry written; prints "RATIO kind x what"."""
    assert np.isfinite(P).all(), f"{what}: {int((~np.isfinite(P)).sum())} entries never written"
    ratio = bound_ratio(P, ref, S, K, scale)
    print(f"RATIO {kind} {ratio:.4f} {what}")
    assert ratio <= 1.0, f"{what}: worst |P - ref| / bound = {ratio:.3f}"


@functools.lru_cache(maxsize=12)
def reference(name, K, dtype, data, seed=0):
    """(A, B, P, S) of pattern `name`: operands as the kernel sees them (read-only, shared by the
    cases of one (pattern, K, dtype)) and their float64 reference. data: "grid", "signed" or
    "identity" (the same for every seed)."""
    pat = pattern(name)
    M, N, _, _ = pat
    if data == "identity":
        A, B = (as_seen(X, dtype) for X in identity_data(M, N, K))
    else:
        gen = {"grid": grid_data, "signed": signed_data}[data]
        A = as_seen(gen(M * K, 101 + 2 * seed), dtype).reshape(M, K)
        B = as_seen(gen(N * K, 202 + 2 * seed), dtype).reshape(N, K)
    P, S = sddmm_ref(pat, A, B)
    for x in (A, B, P, S):
        x.setflags(write=False)
    return A, B, P, S


# kind: the launch (csrc/launch_select.hpp Launch): colmajor (fp32), half (column-major fp16/bf16),
# rowblock, dense, ptile. proof: {evidence: value} checked by check_stats on top of the kind's own
# evidence: rb_pairs / rb_batches / rb_orig_rows / rb_col_blocks (the stats bit of the row size set
# or clear), rb_tiles (kept tiles > 0), rb_rows (rows per block), nt (threads per workgroup, from
# the layout's geometry), store (how P is written: "direct", "runs" or "positions"; default: runs
# for out_staged = 1, else direct). need: a property of the plan the case relies on ("tiles": dense tiles
# and a residual, "no_tiles", "no_residual").
Case = collections.namedtuple("Case", "name kind pattern K dtype layout tuning proof need")


def rb_slot(K, dtype):
    """Plan.stats() index of the row size of (K, dtype): rows of 128 B .. 2 KiB -> 0 .. 4."""
    return {128: 0, 256: 1, 512: 2, 1024: 3, 2048: 4}[K * (4 if dtype == F32 else 2)]


# rows per block that put the A image over 80 KiB (1024 threads, one workgroup per CU) per row
# size; 16 rows keep it under (512 threads). csrc/rb_schedule.cpp rb_geometry
RB_ROWS_NT1024 = {0: 1024, 1: 512, 2: 288, 3: 144, 4: 64}


def _cases():
    out = []

    def add(name, kind, pat, K, dtype, layout="auto", tuning=None, proof=None, need=None):
        out.append(Case(f"{name}_K{K}_{DTYPE_NAME[dtype]}", kind, pat, K, dtype, layout,
                        dict(tuning or {}), dict(proof or {}), need))

    # column-major fp32: K without a row-block row size under the auto rule, the others forced
    for K in (16, 48, 96, 192, 1024):
        add("cm", "colmajor", "zipf", K, F32, need="tiles")
    for K in (32, 64, 128, 256, 512):
        add("cm", "colmajor", "zipf", K, F32, layout="colmajor", need="tiles")
    add("cm_residual_only", "colmajor", "empty", 64, F32, layout="colmajor", need="no_tiles")
    add("cm_residual_only", "colmajor", "hub", 48, F32, need="no_tiles")
    add("cm_blocky", "colmajor", "blocky", 128, F32, need="no_residual")
    # column-major fp16 / bf16
    for dtype in (F16, BF16):
        for K in (32, 96):
            add("half", "half", "zipf", K, dtype, need="tiles")
        for K in (128, 512):
            add("half", "half", "zipf", K, dtype, layout="colmajor", need="tiles")
        add("half_residual_only", "half", "empty", 32, dtype, need="no_tiles")
        add("half_blocky", "half", "blocky", 128, dtype, tuning={"ptile": 0}, need="no_residual")
    # row-block, every row size (the default form: lite for fp32, kept MFMA tiles for the halves)
    for K in (32, 64, 128, 256, 512):
        add("rb", "rowblock", "zipf", K, F32)
    for K, dtypes in ((64, (F16,)), (128, (BF16,)), (256, (F16, BF16)), (512, (F16,)),
                      (1024, (F16, BF16))):
        for dtype in dtypes:
            add("rb", "rowblock", "zipf", K, dtype)
    add("rb_empty", "rowblock", "empty", 64, F32)
    add("rb_hub", "rowblock", "hub", 128, BF16)
    # row-block forms at 512-byte rows (pairs need >= 512 B, batches <= 512 B, and no kept tile)
    for K, dtype, base in ((128, F32, {}), (256, BF16, {"tile_min_half": 257})):
        forms = [
            ("staged", {"out_staged": 1}, {"rb_pairs": False}),
            ("pairs", {"out_staged": 1, "pair_min_items": 0}, {"rb_pairs": True}),
            ("batches", {"batches": 1}, {"rb_batches": True}),
            ("batches_staged", {"out_staged": 1, "batches": 1}, {"rb_batches": True, "rb_pairs": False}),
            ("batches_pairs", {"out_staged": 1, "pair_min_items": 0, "batches": 1},
             {"rb_pairs": True, "rb_batches": True}),
            ("orig_rows", {"orig_rows": 1}, {"rb_orig_rows": True}),
            ("col_blocks", {"col_blocks": 1}, {"rb_col_blocks": True}),
            ("l2_range", {"l2_range_kb": 64}, {}),
            ("rb_rows16", {"rb_rows": 16}, {"rb_rows": 16, "nt": 512}),
            ("unpacked", {"out_packed": 0}, {}),
        ]
        for form, knobs, proof in forms:
            add("rb_" + form, "rowblock", "zipf", K, dtype, tuning=dict(base, **knobs), proof=proof)
    # kept tiles on MFMA in the row-block kernel
    add("rb_tiles", "rowblock", "zipf", 128, F32, tuning={"tile_min_f32": 0}, proof={"rb_tiles": True})
    add("rb_tiles", "rowblock", "zipf", 256, F16, tuning={"tile_min_half": 0}, proof={"rb_tiles": True})
    add("rb_tiles_blocky", "rowblock", "blocky", 64, F32, layout="rowblock",
        tuning={"tile_min_f32": 0}, proof={"rb_tiles": True})
    add("rb_tiles_blocky", "rowblock", "blocky", 512, BF16, layout="rowblock",
        tuning={"tile_min_half": 0}, proof={"rb_tiles": True})
    # pick_rb's whole product: dtype x row size x workgroup size x {lite, full} x {fixed phases,
    # dynamic batches (rows <= 512 B)}, and the pair kernel (rows >= 512 B; with batches at 512 B).
    # full = staged output (not lite); no kept tile, so that lite and pairs are what the knobs say
    for dtype in (F32, F16, BF16):
        for slot in range(5):
            K = (128 << slot) // (4 if dtype == F32 else 2)
            for nt in (512, 1024):
                pat = "tall" if (slot == 0 and nt == 1024) else "zipf"
                base = {"rb_rows": 16 if nt == 512 else RB_ROWS_NT1024[slot], "tile_min_half": 257,
                        "pair_min_items": 1 << 30, "batches": 0}
                forms = [("lite", {}, {}), ("full", {"out_staged": 1}, {})]
                if slot <= 2:
                    forms += [("lite_dyn", {"batches": 1}, {"rb_batches": True}),
                              ("full_dyn", {"out_staged": 1, "batches": 1}, {"rb_batches": True})]
                if slot >= 2:
                    forms += [("pair", {"out_staged": 1, "pair_min_items": 0}, {"rb_pairs": True})]
                if slot == 2:
                    forms += [("pair_dyn", {"out_staged": 1, "pair_min_items": 0, "batches": 1},
                               {"rb_pairs": True, "rb_batches": True})]
                for form, knobs, proof in forms:
                    proof = dict({"rb_pairs": False, "rb_batches": False, "nt": nt}, **proof)
                    add(f"rbx_{form}_nt{nt}", "rowblock", pat, K, dtype, tuning=dict(base, **knobs),
                        proof=proof)
    # dense-sampled
    for dtype in (F16, BF16):
        for K in (64, 320):
            add("dense", "dense", "uniform300", K, dtype)
    # k_sddmm_dense<DT, 64, NS, NW>: four waves (dense_ks = 1; NS = 2 only), eight waves (the default
    # under 512 tiles) at every ring depth NS = 2 (above) .. 5, five chunks so that the ring wraps
    for dtype in (F16, BF16):
        for K in (64, 320):
            add("dense_ks1", "dense", "uniform300", K, dtype, tuning={"dense_ks": 1})
        for ns in (3, 4, 5):
            add(f"dense_ns{ns}", "dense", "uniform300", 320, dtype, tuning={"dense_ns": ns})
    # panel-tile, k_sddmm_ptile<BF16, NK, W>: every dtype and K at four waves (ptile_tpi <= 4; items of
    # up to 3 tiles) and eight (items of up to 8 tiles: every wave busy; up to 17 on `blockmask768`:
    # more tiles than waves, the per-wave tile loop), one tile per item (tpi = 1, and the default
    # equal runs when the tiles are fewer than the CUs), and the default runs on `blockmask768`
    # (more tiles than CUs: runs of two tiles, some across a panel boundary with both panels' A
    # rows). ptile proofs are checked against the plan's blockOffsets (ptile_item_list)
    for dtype in (F16, BF16):
        for K in (64, 128, 256, 512):
            add("ptile", "ptile", "blockmask", K, dtype, need="no_residual", proof={"ptile_max_tiles": 1})
            add("ptile_tpi3", "ptile", "blockmask", K, dtype, tuning={"ptile_tpi": 3}, need="no_residual",
                proof={"ptile_max_tiles": 3})
            add("ptile_tpi8", "ptile", "blockmask", K, dtype, tuning={"ptile_tpi": 8}, need="no_residual",
                proof={"ptile_max_tiles": 8})
            add("ptile_tpi64", "ptile", "blockmask768", K, dtype, tuning={"ptile_tpi": 64},
                need="no_residual", proof={"ptile_max_tiles": 17})
            add("ptile_runs", "ptile", "blockmask768", K, dtype, need="no_residual",
                proof={"ptile_two_panels": True})
        add("ptile_tpi1", "ptile", "blockmask", 128, dtype, tuning={"ptile_tpi": 1}, need="no_residual",
            proof={"ptile_max_tiles": 1})
    add("ptile_residual", "ptile", "zipf", 128, F16, tuning={"ptile": 1}, need="tiles")
    add("ptile_residual", "ptile", "zipf", 256, BF16, tuning={"ptile": 1}, need="tiles")
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# one case per launch kind for the other entry points, the guard zones and the non-finite tests
ONE_PER_KIND = ["cm_K48_f32", "half_K96_f16", "rb_K128_f32", "rb_K256_bf16", "dense_K64_bf16",
                "ptile_K64_f16", "ptile_residual_K128_f16"]
# bsmr_sddmm_panels: the row-block kernel over a range's own layout (fp32, half, and a plan whose
# whole launch is dense-sampled), and every reachable k_sddmm_panels_f32<KT, G> (the same (KT, G) as
# the whole-plan kernel: generic KT at G = 4 / 8 / 16, KT = 32 at G = 8, KT = 64 .. 512 at G = 16;
# tiles only on `blocky`)
PANEL_CASES = ["rb_K128_f32", "rb_K256_bf16", "rb_pairs_K128_f32", "dense_K64_bf16", "cm_K16_f32",
               "cm_K48_f32", "cm_K96_f32", "cm_K192_f32", "cm_K1024_f32", "cm_K32_f32", "cm_K64_f32",
               "cm_K128_f32", "cm_K256_f32", "cm_K512_f32", "cm_blocky_K128_f32"]


def ptile_item_list(block_offsets, tpi, cus):
    """The panel-tile launch's items (first panel, second panel, tiles, tiles of the first panel) as
    csrc/sddmm_half.hip build_ptile_layout documents them: tpi > 0: every panel's n tiles in
    ceil(n / tpi) near-equal items; tpi = 0: the T tiles in max(cus, ceil(T / 8)) equal runs, a run
    that crosses a panel boundary taking both panels (split before a third)."""
    bo = [int(x) for x in block_offsets]
    npan, T = len(bo) - 1, bo[-1]
    items = []
    if tpi > 0:
        for q in range(npan):
            a, n = bo[q], bo[q + 1] - bo[q]
            k = -(-n // tpi)
            for i in range(k):
                nt = n * (i + 1) // k - n * i // k
                items.append((q, q, nt, nt))
        return items
    panel_of = lambda t: int(np.searchsorted(bo, t, side="right")) - 1  # noqa: E731
    nb = max(cus, -(-T // 8))
    for k in range(nb if T else 0):
        t, e = T * k // nb, T * (k + 1) // nb
        while t < e:
            q0 = panel_of(t)
            e0 = min(bo[q0 + 1], e)
            if e0 == e:
                items.append((q0, q0, e - t, e - t))
                t = e
            else:
                q1 = panel_of(e0)
                e1 = min(bo[q1 + 1], e)
                items.append((q0, q1, e1 - t, e0 - t))
                t = e1
    return items


def plan_kwargs(case):
    return dict(alpha=0.3, delta=0.3, free_mem_bytes=FREE, layout=case.layout, tuning=case.tuning)


def check_stats(case, st, launch, geom=None, store=None):
    """Failures (strings) of the evidence that `case` ran the path it names. st: Plan.stats() after
    the launch; launch: gpu_util.plan_launch, the library's account of the launch and of the
    row-block kernel's form; geom: gpu_util.rb_geometry of the launched layout (needed by an `nt`
    proof), or for the panel-tile launch dict(block_offsets=the plan's blockOffsets, cus=the
    device's CU count); store: gpu_util.rb_store of the launched row-block layout (how it
    writes P: the staged cases are held to the store form they in fact run, a `store` proof)."""
    bad = []

    def want(cond, what):
        if not cond:
            bad.append(f"{case.name}: {what}")

    if case.need == "tiles":
        want(st["num_dense_tiles"] > 0 and st["num_residual"] > 0, "pattern needs tiles and a residual")
    elif case.need == "no_tiles":
        want(st["num_dense_tiles"] == 0, "pattern must have no dense tile")
    elif case.need == "no_residual":
        want(st["num_dense_tiles"] > 0 and st["num_residual"] == 0, "pattern must be tiles only")
    want(launch["kind"] == case.kind, f"the library runs the {launch['kind']} launch, not {case.kind}")
    built = dict(rowblock=any(st["rb_items"]), dense=st["dense_sampled_tiles"] > 0,
                 ptile=st["ptile_items"] > 0)
    for kind, on in built.items():
        want(on == (kind == case.kind), f"the {kind} layout is {'' if on else 'not '}built: "
                                        f"not the {case.kind} launch")
    if case.kind == "ptile" and case.proof:
        # the item list the documented rule gives has the layout's slot count (8 lists, padded),
        # and holds what the case is there for
        want(geom is not None, "a panel-tile proof needs the plan's blockOffsets")
        items = ptile_item_list(geom["block_offsets"], case.tuning.get("ptile_tpi", 0), geom["cus"]) if geom else []
        want(st["ptile_items"] == -(-len(items) // 8) * 8, f"ptile_items {st['ptile_items']}: the rule gives "
                                                          f"{len(items)} items")
        most = max([it[2] for it in items], default=0)
        if "ptile_max_tiles" in case.proof:
            want(most == case.proof["ptile_max_tiles"], f"largest item holds {most} tiles")
        if case.proof.get("ptile_two_panels"):
            want(any(it[0] != it[1] for it in items), "no item spans two panels")
            want(most >= 2, "no item of two tiles")
    if case.kind != "rowblock":
        return bad
    slot = rb_slot(case.K, case.dtype)
    bit = 1 << slot
    want([i for i, n in enumerate(st["rb_items"]) if n] == [slot],
         f"rb_items {st['rb_items']}: not slot {slot} alone")
    proof = dict(case.proof)
    proof.setdefault("rb_col_blocks", False)  # off unless asked for
    if "pair_min_items" not in case.tuning:
        proof.setdefault("rb_pairs", False)  # the suite's patterns stay under the default 4096 items
    for f in ("rb_pairs", "rb_batches", "rb_orig_rows", "rb_col_blocks"):
        if f in proof:  # (else the auto rule decides: batches at 512-byte rows, original rows)
            want(bool(st[f] & bit) == proof[f], f"{f} bit {slot} is {'not ' if proof[f] else ''}set")
    # tiles are kept from tile_min entries on (default: fp32 257 = never, half 128); without a kept
    # tile the lite kernel and the pairs are what the other knobs say
    f32 = case.dtype == F32
    if case.tuning.get("tile_min_f32" if f32 else "tile_min_half", 257 if f32 else 128) >= 257:
        proof.setdefault("rb_tiles", False)
    if "rb_tiles" in proof:
        want((st["rb_tiles"][slot] > 0) == proof["rb_tiles"], f"rb_tiles[{slot}] = {st['rb_tiles'][slot]}")
    if "rb_rows" in proof:
        want(st["rb_rows"][slot] == proof["rb_rows"], f"rb_rows[{slot}] = {st['rb_rows'][slot]}")
    if "nt" in proof:
        want(geom is not None and geom["nt"] == proof["nt"], f"geometry {geom}: not {proof['nt']} threads")
    # the kernel form the launch took (csrc/launch_select.cpp rb_form), against what the case names
    if launch["kind"] != "rowblock":
        return bad
    want(launch["slot"] == slot, f"launch slot {launch['slot']}, not {slot}")
    for f, key in (("rb_pairs", "pairs"), ("rb_batches", "dyn")):
        want(launch[key] == bool(st[f] & bit), f"launch {key} = {launch[key]} against the stats bit")
        if f in proof:
            want(launch[key] == proof[f], f"launch {key} = {launch[key]}")
    if geom is not None:
        want(launch["NT"] == geom["nt"], f"launch NT = {launch['NT']} against the geometry's {geom['nt']}")
    if "nt" in proof:
        want(launch["NT"] == proof["nt"], f"launch NT = {launch['NT']}")
    want(launch["grid"] == st["rb_items"][slot] // (2 if launch["pairs"] else 1),
         f"launch grid {launch['grid']} of {st['rb_items'][slot]} items")
    # lite: no kept tile, direct stores (the suite's outputs stay under the 8 MiB of the staged
    # auto rule, so staged means out_staged = 1), default staging policy, late B, no diag bit
    lite = (st["rb_tiles"][slot] == 0 and case.tuning.get("out_staged") != 1 and
            not any(k in case.tuning for k in ("stage_nt", "late_b", "diag")))
    if case.name.startswith("rbx_"):
        named = case.name.startswith("rbx_lite")
        want(lite == named, f"the case's knobs give lite = {lite}, its name {named}")
    want(launch["lite"] == lite, f"launch lite = {launch['lite']}, the case names {lite}")
    want(not (launch["lite"] and launch["pairs"]), "a launch both lite and paired")
    # how P is written: direct stores, or staged through LDS slots and then by the
    # run table ("runs") or by per-result positions ("positions"). The suite's patterns are
    # column-sorted unless a case says otherwise, so no item has more runs than threads and every
    # staged case (`rb_staged_*`, `rb_pairs_*`, `rb_batches_staged_*`, `rbx_full_*`, `rbx_pair_*`)
    # runs the run table; pairs exist only with it (csrc/launch_select.cpp rb_form)
    if store is not None:
        staged = case.tuning.get("out_staged") == 1
        form = "direct" if not store["outLds"] else "runs" if store["outRuns"] else "positions"
        named = proof.get("store", "runs" if staged else "direct")
        want(form == named, f"P is written by {form}, the case names {named} "
                            f"(outLds {store['outLds']}, outCap {store['outCap']}, outRuns {store['outRuns']})")
        want(store["NT"] == launch["NT"], f"store export NT {store['NT']} against the launch's {launch['NT']}")
        want(not launch["pairs"] or form == "runs", "a paired launch without a run table")
        if form == "direct":
            want(store["outPacked"] == launch["packed"], "packed output against the launch's account")
        if form == "runs":
            real = store["real"]
            want(int(store["nruns"][real].max(initial=0)) <= store["NT"], "an item with more runs than threads")
            want(int(store["longest"][real].max(initial=0)) <= 64, "a run longer than a wave")
            want(((store["nruns"][real] > 0) == (store["ent"][real] > 0)).all(), "an item with entries and no run")
    return bad
