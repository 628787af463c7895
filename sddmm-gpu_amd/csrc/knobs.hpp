// knobs.hpp — a plan's tuning, resolved: every value that bsmr_plan_options and bsmr_tuning
// (include/bsmr.h) set, with its one default and the measurement behind it, and the rules that
// map the two structs onto it. Standard library and bsmr.h only: no HIP, no device, so it builds,
// runs and is tested on a machine without a GPU. A Plan holds one Knobs (Plan::k); the host-only
// units (rb_schedule.hpp, launch_select.hpp) read the same struct. A new knob is a field of
// bsmr_tuning, a row of the field table in knobs.cpp, a member here and a rule in apply_tuning.
#pragma once

#include <cstdint>

#include "bsmr.h"
#include "verdict.hpp"

namespace bsmr {

constexpr uint32_t RB_PIECE_MAX = 16;  // entries per column-run piece (row-block layout)

struct Knobs {
    // launch layout (bsmr_plan_options.layout): row-block LDS items for K in {64, 128, 256, 512}
    // unless BSMR_LAYOUT_COLMAJOR; the column-major residual slots for every other K
    bool use_rowblock = true;
    bool force_rowblock = false;  // BSMR_LAYOUT_ROWBLOCK: also for tile-dominated plans
    uint32_t rb_lds_kb = 144;  // LDS budget of a row-block workgroup (bsmr_plan_options.lds_budget_kb)
    bool rb_lds_user = false;  // set by the caller: then also for staged layouts
    // staged-output layouts (below) default to a 120 KiB image and 4 MiB column ranges: the
    // 40 KiB tail holds 10240 results, so items are cut less, and each row block is staged for
    // half as many ranges. C4 reddit-like x0.5 sweep (profiles/r02abl/C4_sweep*.txt): 1.305 ms at
    // (144 KiB, 2 MiB) -> 1.128 ms at (120 KiB, 4 MiB); C3 unchanged (72.9-73.2 us)
    uint32_t rb_lds_kb_staged = 120, l2_range_kb_staged = 4096;
    uint32_t diag = 0;  // BSMR_DIAG profiling ablations (wrong results; never set in normal use)
    // L2 budget of one column range of the row-block layout (KiB; BSMR_L2_RANGE_KB)
    uint32_t l2_range_kb = 2048;
    bool l2_range_user = false;  // BSMR_L2_RANGE_KB given: then also for staged layouts
    // entries per column-run piece of the row-block layout (<= RB_PIECE_MAX; BSMR_PIECE_MAX)
    uint32_t piece_max = RB_PIECE_MAX;
    // a column-run piece's weight in the item cost model, in entries (BSMR_PIECE_WEIGHT): each
    // piece gathers a whole B row. Measured (profiles/r02c/piece_weight.txt): C2 11.60 us at 1,
    // 11.05 at 4, 11.15 at 8 (items of the short last row block, all short pieces, were the
    // launch's tail); C4 x0.5 -0.8 %; C3 unchanged
    double piece_weight = 4.0;
    // the same weight in the row-panel shard cost (RowBlockLayout::rbCost, bsmr_plan_shard):
    // BSMR_SHARD_PIECE_WEIGHT
    double shard_piece_weight = 4.0;
    // row-block results staged in LDS and written in CSR order per item, for P larger than
    // out_staged_min bytes (BSMR_OUT_STAGED: 0 never, 1 always, else auto). Measured
    // (profiles/r02ab1): C3 cop20k-like (P 10 MB) 77.0 -> 72.0 us, C4 reddit-like x0.5 (232 MB)
    // 1.394 -> 1.305 ms; C2 nips-like (3 MB, P stays in L2 and its scattered stores merge there)
    // 11.86 -> 12.60 us, so it stays on one store per entry
    int out_staged = -1;
    // BSMR_OUT_PACKED: unstaged row-block layouts carry the CSR position in the metadata word
    // (0 never, else whenever nnz <= 2^22)
    int out_packed = -1;
    // A staging with the nt cache policy (BSMR_STAGE_NT: 1 always, 0 never; auto = never)
    int stage_nt = -1;
    int rb_rows_force = -1;  // BSMR_RB_ROWS: rows per row block (tuning / experiments)
    // BSMR_LATE_B: phase-0 B loads after the staging barrier (0 = behind the LDS-DMAs, else on).
    // Measured (profiles/r03d/ab_lateb): C2 11.05 -> 10.86 us, C3 72.0 -> 68.9, C4 x0.5 1.012 ->
    // 0.998 ms, C5 unchanged
    int late_b = -1;
    // item cost cap (multiple of one slot's share of a round; 0 = none), cost-even chunk cuts and
    // list-scheduled (heaviest-first) unsplit items; item_fixed = an item's fixed cost in entries
    // beside its staged rows (piece_weight each). BSMR_ITEM_CAP / BSMR_ITEM_SCHED
    double item_cap = -1.0;  // < 0: auto (build_rowblock_layout), 0: no cap
    bool item_cost_cuts = true, item_lpt = true;
    double item_fixed = 1024.0;
    // sparse-row patterns with fewer row blocks than slots: one block per workgroup slot
    bool small_sparse_rb = true;
    uint64_t out_staged_min = 8ull << 20;
    // fp16/bf16 patterns with at least this fraction of M x N stored run the dense-sampled
    // launch (whole 128 x 128 MFMA tiles; BSMR_DENSE_MIN; > 1 = never). Measured crossover
    // (tools/dense_sweep.py, 2048^2 bf16 K=512): gathered faster at 3 %, dense from 5 %
    float dense_min = 0.05f;
    // clusters per persistent clustering launch (bsmr_plan_options.cluster_batch); r01k timing
    // on reddit_like x0.25: 512 -> 9.7 s, 4096 -> 4.6 s, 16384 -> 2.3 s (fewer host round trips, more in flight)
    uint32_t cluster_batch = 16384;
    // clustering candidate filter (cluster_filter.hip; bsmr_tuning.cluster_filter): -1 auto (M >=
    // filter_min_rows, alpha >= 0.01, the filter's buffers fit a quarter of the free memory), 0
    // never, 1 whenever alpha >= 0.01 and it fits
    int cluster_filter = -1;
    uint32_t filter_min_rows = 32768;
    // staged-output row-block layouts (rows >= 512 B) of at least this many items run in pairs
    // (k_sddmm_rb_pair; bsmr_tuning.pair_min_items)
    uint32_t pair_min_items = 4096;
    // dynamic piece batches of the row-block launch (rows of <= 512 B; bsmr_tuning.batches): 1
    // always, 0 never, -1 for 512-byte rows whose items hold >= batch_min_phases pieces per
    // row-group on average
    int batches = -1;
    double batch_min_phases = 2.0;
    // static piece order of row-block items without dynamic batches (rb_schedule.cpp balance_pieces;
    // bsmr_tuning.piece_balance): 1 = runs dealt to the least-loaded wave, 0 = longest first in
    // position order
    int piece_balance = 0;
    // whole-plan original-order candidates (Plan::rblo) are built for sparse-row patterns and
    // used when their column-run pieces are below 0.9 x the reordered layout's pieces + 16 per
    // MFMA tile. BSMR_ORIG_ROWS: 0 = never, 1 = always, else auto
    int orig_rows = -1;
    // whole-plan column-block layouts (Plan::rblc). BSMR_COL_BLOCKS: 0 =
    // never (default: on C2, the one wide BASELINE pattern, 19 % fewer pieces measured 1 % slower
    // at steady state and 0-4 % faster from a standing start), 1 = always, 2 = for
    // wide patterns (N >= 2 M) whose column-block pieces are below 0.9 x the chosen layout's
    int col_blocks = 0;
    // BSMR_ORIG_CONTIG: unsplit original-order blocks dealt as contiguous eighths per XCD (1)
    // or to the shortest list (0); C3: 78.6 -> 76.8 us (profiles/r01s)
    int orig_contig = 1;
    // stored entries a dense tile needs to run on MFMA in the row-block launch (BSMR_TILE_MIN_F32
    // / BSMR_TILE_MIN_HALF); 0 = every tile. Measured (r01k sweep, profiles/r01k/tile_min.json):
    // fp32 MFMA (16x16x4) runs at the vector-FMA rate on gfx950 and a tile pays its empty slots,
    // so every fp32 tile is cheaper as residual entries (257: none kept; C2 14.4 -> 12.9 us);
    // fp16/bf16 MFMA is 8x the v_dot2 rate, so half tiles stay unless under half full
    uint32_t tile_min_f32 = 257, tile_min_half = 128;
    // BSMR_DENSE_KS: dense-sampled workgroups of 1 = four waves (64 x 64 quadrants), 2 = eight
    // waves (64 x 32 blocks), else eight below 512 non-empty tiles
    int dense_ks = 0;
    int dense_ns = 2;  // BSMR_DENSE_NS: LDS stages of the eight-wave dense launch (2..5)
    int ptile_mode = -1;  // BSMR_PTILE: 0 never, 1 whenever it applies, -1 auto
    // BSMR_PTILE_TPI: 0 = equal tile runs, one per CU (up to two panels each); n > 0 = items of
    // at most n tiles of one panel (C5 block: 4 -> 5.93 us, 2 -> 7.5, 5 -> 7.7)
    uint32_t ptile_tpi = 0;
};

// the launch-layout knobs of t onto k; a field at "auto" keeps k's value. diag is always copied
void apply_tuning(Knobs& k, const bsmr_tuning& t);
// cluster_batch, layout, lds_budget_kb and (when given) the tuning of o onto k: BSMR_ERR_INVALID
// for a layout or LDS budget out of range
Verdict apply_options(Knobs& k, const bsmr_plan_options& o);

}  // namespace bsmr
