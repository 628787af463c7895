"""Patterns, the case table and an independent float64 reference for the plan builder's row
clustering (csrc/plan.hip k_encode / k_cluster, cluster_filter.hip). No GPU
here: tests/test_plan_cases_cpu.py checks this module against the CPU oracle,
tests/test_gpu_plan_sweep.py runs every case on the device.

What a case is meant to reach, by the geometry the builder derives from (M, N, free memory):
  bs   = calculateBlockSize (16 for N <= 98304 unless M * M * 4 exceeds bs * free / 2)
  nbpr = ceil(N / bs) column blocks per row
  B    = 32 * ceil((nbpr / 4) / 32), 32 .. 1024: the reference's clustering block size. Its block
         reduction adds warp w + stride into warp w for stride = B / 64, B / 128, .. 1, so for a
         warp count that is no power of two only some warps reach the result (kept_warps); the
         blocks of the other warps take no part in the norms or the similarity
  T    = clusters per tile: as many representatives of NP = nbpr rounded up to 4 words as fit
         148 KiB, even, at most 8 (8 up to nbpr 4736, 6 from 4737)
Every tree-shape case uses N = 16 nbpr - 3 with nbpr = 128 W - 5 (31 for W = 1), which gives
B = 32 W at block size 16.

first_fit_f64 restates the operation from the reference's source (rowReordering.cu
calculateDispersion, calculate_similarity_norm_weighted_jaccard, bsa_clustering,
get_permutation_gpu; cudaUtil.cuh reduce_sum) in numpy float64. It does not emulate the fp32
summation tree, so it decides like the reference only where no similarity it meets lies near
alpha: it returns the smallest |similarity - alpha|, and a case is "clear" when that exceeds
CLEAR_GAP (the fp32 tree stays within 3e-6 of the real value). The `mutate`
argument breaks one rule at a time; test_plan_cases_cpu.py shows that each mutation changes the
permutation on the cases aimed at it, i.e. that the cases can tell a subtly wrong builder.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

FREE = 288 * 1024 ** 3   # free memory of the other parity tests: block size from N alone
CLEAR_GAP = 1e-4
REF_MAX_SHMEM = 49152    # the reference's maxSharedMemoryPerBlock (calculateBlockSize)
CL_LDS_BUDGET = 148 * 1024


# ------------------------------------------------------------------------------ geometry ----
def block_size(M, N, free_mem):
    """calculateBlockSize in exact integer arithmetic (the table's cases sit far from the fp32
    rounding of the reference's expression; test_plan_cases_cpu.py compares with the oracle)."""
    gmem = -(-(M * M * 4) // (free_mem // 2))
    smem = -(-(N * 4) // (REF_MAX_SHMEM // 2))
    return max(gmem, smem, 16)


def cluster_block_dim(nbpr):
    if nbpr < 32:
        return 32
    return min(1024, max(32, 32 * -(-(nbpr // 4) // 32)))


def tile_clusters(nbpr):
    NP = (nbpr + 3) // 4 * 4
    return max(2, min(8, CL_LDS_BUDGET // (NP * 4)) // 2 * 2)


def kept_warps(B):
    """Warps of a B-thread block whose partial sums reach shm[0] in reduce_sum: the stride loop
    `for (stride = B / 64; stride >= 1; stride >>= 1) if (warp < stride) shm[warp] += shm[warp +
    stride]`, run here on indicator vectors."""
    W = B // 32
    shm = np.eye(W, dtype=np.int64)
    stride = B // 64
    while stride >= 1:
        for w in range(stride):
            shm[w] += shm[w + stride]
        stride >>= 1
    return shm[0] > 0


def kept_blocks(nbpr, B, all_kept=False):
    """Per column block i: thread i mod B adds it, so it counts when that thread's warp is kept."""
    if all_kept:
        return np.ones(nbpr, bool)
    return kept_warps(B)[(np.arange(nbpr) % B) // 32]


def n_for(nbpr, bs=16):
    return bs * nbpr - 3


def nbpr_for_warps(W):
    return 31 if W == 1 else 128 * W - 5


# ------------------------------------------------------------------------------ patterns ----
def _csr_from_rows(M, N, rows):
    lens = np.array([len(r) for r in rows], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    ci = (np.concatenate([np.asarray(r, np.int64) for r in rows]) if lens.sum()
          else np.zeros(0, np.int64))
    assert ci.size == 0 or (ci.min() >= 0 and ci.max() < N)
    return M, N, rp, ci.astype(np.uint32)


def _entries(rng, blocks, counts, bs, N):
    """Sorted columns: counts[k] distinct columns inside column block blocks[k]."""
    cols = []
    for b, k in zip(blocks, counts):
        width = min(bs, N - int(b) * bs)
        cols.append(int(b) * bs + rng.choice(width, size=min(int(k), width), replace=False))
    return np.sort(np.concatenate(cols))


def planted(M, nbpr, bs, seed, empty=None, shuffle=False, masked=None):
    """8 groups of rows; a row draws 16 of its group's 24 base column blocks and 4 noise blocks,
    1 - 3 entries per block. `empty` rows (default 5 %) hold nothing. masked = (row mask, blocks):
    those rows draw 20 blocks from `blocks` instead. shuffle: the columns of each row in random
    order."""
    rng = np.random.default_rng(seed)
    N = n_for(nbpr, bs)
    pool = np.arange(nbpr)
    base = [rng.choice(pool, size=min(24, len(pool)), replace=False) for _ in range(8)]
    n_empty = int(round(0.05 * M)) if empty is None else int(empty)
    is_empty = np.zeros(M, bool)
    is_empty[rng.choice(M, size=n_empty, replace=False)] = True
    rows = []
    for r in range(M):
        g = int(rng.integers(8))
        if masked is not None and masked[0][r]:
            blocks = rng.choice(masked[1], size=min(20, len(masked[1])), replace=False)
        else:
            blocks = np.union1d(rng.choice(base[g], size=min(16, len(base[g])), replace=False),
                                rng.choice(pool, size=4, replace=False))
        cols = _entries(rng, blocks, rng.integers(1, 4, size=len(blocks)), bs, N)
        if shuffle:
            cols = rng.permutation(cols)
        rows.append(cols if not is_empty[r] else cols[:0])
    return _csr_from_rows(M, N, rows)


def windows(M, nbpr, bs, seed, width):
    """M windows of `width` consecutive column blocks with one entry in each, window k one block
    further than window k - 1 (wrapping at the last block that leaves room). Two neighbouring
    windows share width - 1 blocks: similarity (width - 1) / (width + 1) in real arithmetic while
    both lie in kept warps. Every row has the same dispersion, so the ascending order is the row
    order. The rows hold the even windows first, then the odd ones: an odd window then meets both
    its neighbours as clusters of one row, and joining one moves it in the permutation. (With the
    windows in their own order the clusters are runs of consecutive rows whatever the decisions,
    and the permutation is the identity at alpha and at alpha minus one ulp alike.)"""
    rng = np.random.default_rng(seed)
    N = n_for(nbpr, bs)
    span = nbpr - width + 1
    starts = np.concatenate([np.arange(0, M, 2), np.arange(1, M, 2)])
    rows = [_entries(rng, (int(k) % span) + np.arange(width), np.ones(width, np.int64), bs, N)
            for k in starts]
    return _csr_from_rows(M, N, rows)


def masked_rows(M, nbpr, bs, seed):
    """`planted`, but a quarter of the rows have all their entries in blocks of dropped warps
    (their kept norm SC is 0: similarity 1 with a representative whose kept norm is 0 too, 0 with
    any other). Needs a B whose warp count is no power of two."""
    keep = kept_blocks(nbpr, cluster_block_dim(nbpr))
    assert not keep.all()
    rng = np.random.default_rng(seed + 7919)
    mask = np.zeros(M, bool)
    mask[rng.choice(M, size=M // 4, replace=False)] = True
    return planted(M, nbpr, bs, seed, masked=(mask, np.nonzero(~keep)[0]))


LONG_BLOCKS = (255, 256, 257, 511, 512, 513, 1025)


def long_pair(nb, alpha):
    """(s, c) for a pair of rows of nb column blocks that share s blocks with c entries in each and
    hold 1 entry in each of their nb - s other blocks: the first (c, s) whose similarity
    c s / (2 (nb - s) + c s) clears alpha by 5e-4 while the same pair with one shared block missing
    from one row falls 5e-4 short of it (every warp kept; norms as fp32 square roots)."""
    def norm(sq):
        return float(np.sqrt(np.float32(sq)))

    for c in (4, 3, 5, 2, 6, 7, 8):
        for s in range(2, nb):
            n1, n2 = norm((nb - s) + c * c * s), norm((nb - s) + c * c * (s - 1))
            whole = c * s / (2 * (nb - s) + c * s)
            short = (c * (s - 1) / n1) / (c * (s - 1) / n2 + c / n1 + (nb - s) / n1 + (nb - s) / n2)
            if whole > alpha + 5e-4 and short < alpha - 5e-4:
                return s, c
    raise ValueError((nb, alpha))


def long_rows(M, nbpr, bs, seed, alpha=0.3):
    """Pairs of rows with 255 .. 1025 distinct column blocks among short `planted` rows. The two
    rows of a pair share their s highest blocks (a range of its own per pair), c entries in each,
    and hold 1 entry in each of their other blocks, which lie below every shared range. The shared
    entries are therefore the last of both sorted encodings (past every 256-entry chunk), and
    (s, c) = long_pair(nb, alpha): where every warp is kept the pair joins, and would not if the
    last block of one row's encoding were lost."""
    rng = np.random.default_rng(seed)
    N = n_for(nbpr, bs)
    _, _, rp, ci = planted(M, nbpr, bs, seed)
    rows = [ci[rp[r]:rp[r + 1]].astype(np.int64) for r in range(M)]
    slots = rng.choice(np.nonzero(np.diff(rp.astype(np.int64)) > 0)[0], size=2 * len(LONG_BLOCKS),
                       replace=False)
    pairs = [long_pair(nb, alpha) for nb in LONG_BLOCKS]
    # own blocks below every pair's shared ones; never the short last block
    low_end = nbpr - 1 - sum(s for s, _ in pairs)
    top = nbpr - 1
    for k, (nb, (s, c)) in enumerate(zip(LONG_BLOCKS, pairs)):
        top -= s
        assert 2 * (nb - s) <= low_end
        low = rng.permutation(low_end)[:2 * (nb - s)]
        for j in range(2):
            own = low[j * (nb - s):(j + 1) * (nb - s)]
            blocks = np.concatenate([own, top + np.arange(s)])
            counts = np.concatenate([np.ones(len(own), np.int64), np.full(s, c)])
            rows[slots[2 * k + j]] = _entries(rng, blocks, counts, bs, N)
    return _csr_from_rows(M, N, rows)


def identical(M, nbpr, bs, seed):
    rng = np.random.default_rng(seed)
    N = n_for(nbpr, bs)
    blocks = rng.choice(nbpr, size=min(12, nbpr), replace=False)
    row = _entries(rng, blocks, rng.integers(1, 4, size=len(blocks)), bs, N)
    return _csr_from_rows(M, N, [row] * M)


def disjoint(M, nbpr, bs, seed):
    """Row i holds blocks 3 i .. 3 i + 2 (rotated by the seed): no two rows share one."""
    rng = np.random.default_rng(seed)
    N = n_for(nbpr, bs)
    assert 3 * M <= nbpr - 1
    order = rng.permutation(M)
    rows = [_entries(rng, 3 * int(order[r]) + np.arange(3), rng.integers(1, 4, size=3), bs, N)
            for r in range(M)]
    return _csr_from_rows(M, N, rows)


GENERATORS = dict(planted=planted, windows=windows, masked_rows=masked_rows, long_rows=long_rows,
                  identical=identical, disjoint=disjoint,
                  shuffled=functools.partial(planted, shuffle=True))


# ---------------------------------------------------------------------------- case table ----
@dataclass(frozen=True)
class Case:
    name: str
    cls: str                 # the class of DESIGN.md 3.1 this case stands for
    pattern: str             # GENERATORS key
    M: int
    nbpr: int
    alpha: float
    seed: int = 1
    bs: int = 16
    args: tuple = ()         # extra generator keywords as (key, value) pairs
    free_mem: int = FREE
    cluster_batch: int = 0
    tie: bool = False        # similarities sit on alpha: the exact fp32 tree decides
    force_filter: bool = False   # also run with the filter forced on where alpha < 0.01
    # evidence (test_plan_cases_cpu.py: equal to the oracle's geometry; the GPU sweep: equal to
    # Plan.export_rows()'s header)
    ev: dict = field(default_factory=dict, compare=False, hash=False)

    @property
    def N(self):
        return n_for(self.nbpr, self.bs)

    @property
    def clear_expected(self):
        return self.pattern in ("planted", "masked_rows", "long_rows", "shuffled") and not self.tie


def _case(name, cls, pattern, M, nbpr, alpha, **kw):
    bs = kw.get("bs", 16)
    free = kw.get("free_mem", FREE)
    N = n_for(nbpr, bs)
    ev = dict(block_size=block_size(M, N, free), num_blocks_per_row=nbpr,
              cluster_block_dim=cluster_block_dim(nbpr), tile_clusters=tile_clusters(nbpr))
    assert ev["block_size"] == bs, (name, ev, bs)
    return Case(name, cls, pattern, M, nbpr, alpha, ev=ev, **kw)


# windows (width, alpha) pairs with (width - 1) / (width + 1) == alpha in real arithmetic
TIES = ((3, 0.5), (2, 1.0 / 3.0), (4, 0.6), (5, 2.0 / 3.0))

# planted / masked / long / shuffled seeds chosen so that the case is clear (smallest
# |similarity - alpha| > CLEAR_GAP) and, for a warp count that is no power of two, so that keeping
# every warp changes the permutation; test_plan_cases_cpu.py asserts both, none is skipped
SEEDS = {
    "tree_planted_W4": 4, "tree_planted_W6": 2, "tree_planted_W7": 6, "tree_planted_W12": 7,
    "tree_planted_W13": 2, "tree_planted_W14": 6, "tree_planted_W16": 2, "tree_planted_W18": 2,
    "tree_planted_W19": 7, "tree_planted_W20": 8, "tree_planted_W21": 3, "tree_planted_W23": 2,
    "tree_planted_W27": 2, "tree_planted_W29": 4, "tree_planted_W30": 2, "tree_planted_W31": 3,
    "nbpr_4736_planted": 10, "nbpr_253_planted": 2, "nbpr_255_planted": 2,
    "win_R255_z0": 4, "win_R255_z9": 12, "win_R256_z9": 12, "win_R257_z9": 12, "win_R513_z0": 4,
    "win_R513_z9": 5, "filter_M127_nbpr191": 4, "filter_M128_nbpr191": 4,
    "filter_M129_nbpr191": 4, "filter_M257_nbpr129": 2, "filter_M257_nbpr191": 2,
    "masked_W3": 4, "masked_W7": 2, "masked_W31": 5, "long_rows_W31": 2, "shuffled_W8": 7,
}


def _build_cases():
    out = []

    def add(name, cls, pattern, M, nbpr, alpha, **kw):
        kw.setdefault("seed", SEEDS.get(name, 1))
        out.append(_case(name, cls, pattern, M, nbpr, alpha, **kw))

    # tree shape: every B = 32 W
    for W in range(1, 33):
        add(f"tree_planted_W{W}", "tree", "planted", 200, nbpr_for_warps(W), 0.3)
        add(f"tree_windows_W{W}", "tree", "windows", 240, nbpr_for_warps(W), 0.5, tie=True,
            args=(("width", 3),))
    for width, alpha in TIES[1:]:   # the other tie pairs, at a dropped-warp and a full tree
        for W in (5, 8):
            add(f"tie_w{width}_W{W}", "tree", "windows", 240, nbpr_for_warps(W), alpha, tie=True,
                args=(("width", width),))
    # nbpr boundaries: T = 8 | 6, NP padding, block size from the memory branch
    for nbpr in (4736, 4737):
        add(f"nbpr_{nbpr}_planted", "nbpr", "planted", 300, nbpr, 0.3)
        add(f"nbpr_{nbpr}_windows", "nbpr", "windows", 240, nbpr, 0.5, tie=True,
            args=(("width", 3),))
    for nbpr in (252, 253, 254, 255):
        add(f"nbpr_{nbpr}_planted", "nbpr", "planted", 200, nbpr, 0.3)
        add(f"nbpr_{nbpr}_windows", "nbpr", "windows", 240, nbpr, 0.5, tie=True,
            args=(("width", 3),))
    add("bs20_memory_branch", "nbpr", "planted", 600, 250, 0.3, bs=20, free_mem=150000)
    # windows of 256 positions, sub-batches of 64: R = M - z around 64, 256, 512
    for R in (63, 64, 65, 255, 256, 257, 513):
        for z in (0, 9):
            add(f"win_R{R}_z{z}", "window", "planted", R + z, 379, 0.3, args=(("empty", z),))
    # tiles and launches: alpha = 1.0, every position its own cluster
    for R in (64, 65):
        for batch in (7, 8, 9, 24, 64):
            add(f"tiles_R{R}_b{batch}", "tiles", "planted", R, 379, 1.0, cluster_batch=batch,
                args=(("empty", 0),))
    add("tiles_identical_one_cluster", "tiles", "identical", 130, 379, 0.5)
    add("tiles_identical_alpha1", "tiles", "identical", 65, 379, 1.0, cluster_batch=8, tie=True)
    add("tiles_disjoint", "tiles", "disjoint", 100, 379, 0.3, cluster_batch=24)
    # alpha
    for alpha in (0.0, 0.005, 0.01):
        add(f"alpha_{alpha}", "alpha", "planted", 200, 379, alpha, force_filter=True)
    # rows without a common block sit on alpha 0 exactly: similarity 0 is not > 0
    add("alpha_0.0_disjoint", "alpha", "disjoint", 100, 379, 0.0, force_filter=True, tie=True)
    add("alpha_1.0", "alpha", "planted", 200, 379, 1.0)
    # filter geometry: 128 x 128 tiles over the positions, K padded to 64
    for M in (127, 128, 129, 257):
        for nbpr in (128, 129, 191):
            add(f"filter_M{M}_nbpr{nbpr}", "filter", "planted", M, nbpr, 0.3, args=(("empty", 0),))
    # rows of dropped warps only, long rows, unsorted columns
    for W in (3, 7, 31):
        add(f"masked_W{W}", "masked", "masked_rows", 200, nbpr_for_warps(W), 0.3)
    add("long_rows_W32", "long", "long_rows", 120, nbpr_for_warps(32), 0.3)
    add("long_rows_W31", "long", "long_rows", 120, nbpr_for_warps(31), 0.3)
    add("shuffled_W5", "shuffled", "shuffled", 300, nbpr_for_warps(5), 0.3)
    add("shuffled_W8", "shuffled", "shuffled", 300, nbpr_for_warps(8), 0.3)
    return out


PLAN_CASES = _build_cases()
BY_NAME = {c.name: c for c in PLAN_CASES}
assert len(BY_NAME) == len(PLAN_CASES)


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(M, N, rowptr, colidx) of a case; callers do not modify the arrays."""
    c = BY_NAME[name]
    M, N, rp, ci = GENERATORS[c.pattern](c.M, c.nbpr, c.bs, c.seed, **dict(c.args))
    assert (M, N) == (c.M, c.N) and len(ci) >= 2
    rp.setflags(write=False)
    ci.setflags(write=False)
    return M, N, rp, ci


def reordered_rows(name):
    """R = M - z: the rows that hold an entry."""
    rp = pattern(name)[2].astype(np.int64)
    return int((np.diff(rp) > 0).sum())


def settings(case):
    """The (cluster_filter, exact_similarity) settings a case runs under: the filter forced off;
    forced on wherever it can run (alpha >= 0.01; every case has R >= 2) or the case asks for it
    regardless; tie cases also with every similarity on the exact fp32 tree (the filter is then
    never built)."""
    out = [("0", False)]
    if np.float32(case.alpha) >= np.float32(0.01) or case.force_filter:
        out.append(("1", False))
    if case.tie:
        out.append((None, True))
    return out


def filter_expected(case, cluster_filter, exact):
    """stats cluster_filter_used under a setting: forced on, not the exact mode, alpha >= 0.01."""
    return int(cluster_filter == "1" and not exact and np.float32(case.alpha) >= np.float32(0.01))


def alpha_below(alpha):
    """alpha lowered by one fp32 ulp."""
    return float(np.nextafter(np.float32(alpha), np.float32(-1.0)))


# ------------------------------------------------------------------- float64 reference ----
MUTATIONS = ("all_kept", "ge", "unstable", "swap_zero", "jaccard")


def first_fit_f64(M, N, rowptr, colidx, bs, alpha, mutate=None):
    """(permutation, clusters, smallest |similarity - alpha| met) of the reference's row
    reordering in float64: dense block histograms, u32 dispersion and its stable ascending order,
    empty rows into cluster 0, the blocks of kept warps only, integer norms taken to fp32 square
    roots, similarity sum(min) / sum(max) of the norm-scaled counts, `> alpha`, sequential first
    fit (a cluster's representative is the sum of its rows). clusters counts cluster 0 when a row
    is empty. mutate: one of MUTATIONS, or None."""
    assert mutate is None or mutate in MUTATIONS
    rp = np.asarray(rowptr, np.int64)
    ci = np.asarray(colidx, np.int64)
    nbpr = -(-N // bs)
    B = cluster_block_dim(nbpr)
    alpha = float(np.float32(alpha))
    H = np.zeros((M, nbpr), np.int64)
    np.add.at(H, (np.repeat(np.arange(M), np.diff(rp)), ci // bs), 1)
    nz = H > 0
    disp = (np.where(nz, bs - H, 0).sum(axis=1) + H.sum(axis=1) * nz.sum(axis=1)) % 2 ** 32
    if mutate == "unstable":
        order = np.lexsort((-np.arange(M), disp))
    else:
        order = np.argsort(disp, kind="stable")
    z = int((disp == 0).sum())
    Hk = H * kept_blocks(nbpr, B, all_kept=mutate == "all_kept")[None, :]

    def norm(sq):   # sqrt((float) u32 sum of squares), as a double
        return np.sqrt((np.asarray(sq) % 2 ** 32).astype(np.float32)).astype(np.float64)

    SC, S1C = (Hk * Hk).sum(axis=1), Hk.sum(axis=1)
    reps = np.zeros((max(M - z, 1), nbpr), np.int64)
    SR = np.zeros(len(reps), np.int64)
    S1R = np.zeros(len(reps), np.int64)
    ncl = 0
    ids = np.zeros(M, np.int64)
    gap = np.inf
    both_zero, one_zero = (0.0, 1.0) if mutate == "swap_zero" else (1.0, 0.0)
    for pos in range(z, M):
        row = order[pos]
        take = ncl
        if ncl:
            cols = np.nonzero(Hk[row])[0]
            Rk = reps[:ncl][:, cols].astype(np.float64)
            y = Hk[row, cols].astype(np.float64)
            rest = (S1R[:ncl] - reps[:ncl][:, cols].sum(axis=1)).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                if mutate == "jaccard":
                    x = Rk
                else:
                    nr = norm(SR[:ncl])
                    x, y, rest = Rk / nr[:, None], y / norm(SC[row]), rest / nr
                sim = np.minimum(x, y[None, :]).sum(axis=1) / \
                    (np.maximum(x, y[None, :]).sum(axis=1) + rest)
            rz, cz = SR[:ncl] % 2 ** 32 == 0, SC[row] % 2 ** 32 == 0
            sim = np.where(rz & cz, both_zero, np.where(rz | cz, one_zero, sim))
            ok = sim >= alpha if mutate == "ge" else sim > alpha
            take = int(np.argmax(ok)) if ok.any() else ncl
            gap = min(gap, float(np.abs(sim[:min(take + 1, ncl)] - alpha).min()))
        if take == ncl:
            ncl += 1
        reps[take] += Hk[row]
        SR[take] = (reps[take] * reps[take]).sum()
        S1R[take] = reps[take].sum()
        ids[pos] = take + 1
    perm = order[np.argsort(ids, kind="stable")][z:]
    return perm.astype(np.uint32), ncl + (1 if z else 0), gap
