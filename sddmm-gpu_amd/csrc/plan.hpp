// plan.hpp — the device-resident BSMR plan (reference BSMR + RPHM, include/BSMR.hpp:21-159).
#pragma once

#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "knobs.hpp"
#include "launch_select.hpp"
#include "rb_schedule.hpp"
#include "softmax_schedule.hpp"
#include "spmm_schedule.hpp"

namespace bsmr {

// SDDMM work-list granularity
constexpr u32 TILES_PER_ITEM = 1;   // dense tiles per wave item
constexpr u32 RES_PER_ITEM = 256;   // residual entries per panel-major wave item (panel ranges)
constexpr u32 CM_PER_ITEM = 64;     // residual entries per column-major wave item (full launch)
constexpr u32 XCD_BUCKETS = 8;      // MI355X XCDs: column bucket -> workgroups b with b % 8

struct Plan;
// A launch entry point, as the lazy layout builders see it: the caller's stream, and the names
// and (K, dtype) of the BSMR_ERR_NOT_PREPARED message (prep = the call that builds the layout)
struct LaunchSite {
    hipStream_t s;
    const char* who;
    const char* prep;
    u32 K;
    int dtype;
};
// A launch whose layout is not built asks before it builds: BSMR_ERR_NOT_PREPARED when at.s is
// capturing, BSMR_ERR_HIP when that query fails, else BSMR_OK (sddmm.hip). Launches whose layout
// is built never call it
int lazy_build_guard(const LaunchSite& at);
// fp16/bf16 SDDMM launch (sddmm_half.hip); mode: 1 dense tiles, 2 residual, 3 both
int launch_half(const Plan& p, const void* dA, const void* dB, u32 K, int dtype, float* dP,
                u32 mode, hipStream_t s, u32 nb = 1);
// fp16/bf16 dense-sampled launch (sddmm_dense.hip): K a multiple of 64. at: the entry point, for
// the guard of a lazy build (null: build without asking)
int launch_dense(const Plan& p, const void* dA, const void* dB, u32 K, int dtype, float* dP,
                 hipStream_t s, u32 nb = 1, const LaunchSite* at = nullptr);
// fp16/bf16 panel-grouped tile launch (sddmm_half.hip): K in {64, 128, 256, 512}; mode as above
int launch_ptile(const Plan& p, const void* dA, const void* dB, u32 K, int dtype, float* dP,
                 u32 mode, hipStream_t s, u32 nb = 1, const LaunchSite* at = nullptr);

// clustering candidate filter (cluster_filter.hip): the bit triangle of pairs (leader q,
// position p > q) whose similarity bound may reach alpha; W = words per full row
int build_sim_filter(const uint4* pmeta, const u32* enc, u32 M, u32 nbpr, u32 B, u32 keptMask, float alpha,
                     DevBuf<u32>& bits, u32& W, hipStream_t s);
u64 sim_filter_words(u32 M);

u32 block_size_for(u32 M, u32 N, u64 free_mem);
u32 cluster_block_dim(u32 nbpr);
u32 kept_warp_mask(u32 B);

struct Plan {
    int device = 0;
    hipStream_t stream = nullptr;
    u32 M = 0, N = 0, nnz = 0;
    u32 bs = 16, nbpr = 1, B = 32, keptMask = 1;
    float alpha = 0.3f, delta = 0.3f;
    int exact_all = 0;
    // every tuning and option value, resolved (knobs.hpp); results and state stay here
    Knobs k;
    bool filter_used = false;
    float filter_ms = 0.f;

    // input
    DevBuf<u32> rowptr, colidx;
    // row stage
    DevBuf<u32> enc, nblk, disp, SC, S1C, asc;
    DevBuf<u32> rows;  // reorderedRows_
    u32 z = 0, R = 0, P = 0;
    int32_t numClusters = 1;
    u64 exact_evals = 0, total_evals = 0;
    float row_ms = 0.f, col_ms = 0.f;

    // column stage (the sorted panel segments do not depend on delta and are kept)
    bool segments_ready = false;
    DevBuf<u32> roff, skeys, svals, ent_idx, seg_begin, seg_end;
    DevBuf<uint8_t> ent_lr;
    DevBuf<u32> denseCols, denseColOffsets, sparseCols, sparseColOffsets, sparseValueOffsets;
    DevBuf<u32> blockOffsets, blockValues, sparseValues, sparseRel, sparseColIdx;
    u32 numDenseTiles = 0, nres = 0, maxTilesPerPanel = 0, numDenseTB = 0, numSparseTB = 0;
    std::vector<u32> h_blockOffsets, h_sparseValueOffsets;

    // work lists
    DevBuf<uint4> denseItems, resItems;
    u32 nDenseItems = 0, nResItems = 0;
    DevBuf<u32> tileRows;  // [tile][16] A-row index of each tile row (NULLV = none)
    // column-major residual execution list (same entries as the reference residual arrays,
    // ordered by (column % 8, column), stable): A row, column, output index; and the
    // XCD-interleaved slots {e0, e1} of the full launch
    DevBuf<u32> cmRow, cmCol, cmOut;
    DevBuf<uint2> cmSlots;
    u32 nSlots = 0;

    // Row-block launch layout for one K (built on first use): the A rows of RB consecutive
    // reordered positions are staged in LDS once per workgroup; residual entries are sorted by
    // (row block, column) so one B read serves a column run. The columns are cut into 8 ranges of
    // equal residual count, one per XCD; item i {rb, t0, t1, e0} (+ itemEnd[i]) holds a chunk of
    // row block rb's entries in column range i % 8 (so its B columns sit in that XCD's L2) and a
    // share of rb's dense tiles; about one item per workgroup slot of the chip.
    // Residual entries of an item are cut into column-run pieces of <= RB_PIECE_MAX entries; the
    // 4-lane row-groups of a workgroup take one piece each per phase, so every group loads its B
    // column in the same (full-width) instruction. items[i].w / itemEnd[i] delimit its pieces.
    struct RowBlockLayout {
        u32 rowBytes = 0, RB = 0, NT = 1024, nRB = 0, nItems = 0, nPieces = 0;
        // panels [pa, pb) covered (the whole plan: 0, P); row block b starts at reordered
        // position 16 * pa + b * RB; rows at or past rowEnd = min(R, 16 * pb) are not staged
        u32 pa = 0, pb = 0, rowEnd = 0;
        // dense tiles run as MFMA tiles only with >= tileMin stored entries; the entries of the
        // others join the residual entries (fp32 MFMA has no rate advantage over vector FMA, so a
        // sparse fp32 tile costs more than its entries' dot products)
        u32 tileMin = 0, nTilesKept = 0, nDemoted = 0, nEntries = 0, nWorkItems = 0;
        DevBuf<u32> tileIds;  // kept tile ids; item tile ranges index this list
        size_t lds = 0;
        DevBuf<u32> meta;   // local row << 22 | column (staged output: local row << 22 | slot)
        DevBuf<u32> out;    // output index (CSR position); released when the output is staged
        // staged output (outLds != 0): an item's results go to LDS at byte offset outLds, slot =
        // the entry's rank by CSR position inside its item, and the workgroup writes them at the
        // end in CSR order (P[sortedPos[ea + t]] = slot t: runs of consecutive positions become
        // full-line stores instead of one scattered 4-byte store per entry). itemEnt[i] = {ea,
        // number of entries} of item i; entries of an item never exceed the LDS tail past the
        // A image (outCap floats)
        u32 outLds = 0, outCap = 0;
        // packed output (unstaged layouts of plans with nnz <= 2^22): the entry metadata's low 22
        // bits hold the CSR position itself, so an entry costs one 4-byte metadata load (no out)
        bool outPacked = false;
        DevBuf<u32> sortedPos;
        DevBuf<uint2> itemEnt;
        // run table (staged output, outRuns): the item's slots in CSR order cut into runs of
        // consecutive positions (one per row it touches when rows are column-sorted): runs[j] =
        // {first position, first slot | length << 16}, itemRuns[i] = {first run, number of runs}
        // (<= NT, one per lane); the store pass then reads 8 bytes per run instead of a position
        // per result, and sortedPos is released
        bool outRuns = false;
        DevBuf<uint2> runs, itemRuns;
        DevBuf<uint4> items;
        DevBuf<u32> itemEnd;
        DevBuf<uint2> pieces;  // {first entry, column | (length - 1) << 22}
        // per row block: Σ over its items of (entries + pieces + 16 tiles + RB staged rows), the
        // shard cost model of bsmr_plan_shard
        std::vector<double> rbCost;
        // per item slot (launch order): {row block, kept tiles, entries, pieces}; padding zeros
        std::vector<uint4> itemStat;
        // original-order row blocks (banded / FEM patterns whose reordering scatters the band):
        // row block b = original rows [b RB, (b + 1) RB), staged through rowIds (identity), every
        // entry residual; whole-plan launches only (shards cut reordered panels)
        bool orig = false;
        // column blocks (wide patterns, Knobs::col_blocks): the roles of A and B swapped — block b
        // = original COLUMNS [b RB, (b + 1) RB), their B rows staged through rowIds (identity over
        // N), and each piece a run of one A row (an original row of S) over the block's columns;
        // the metadata's "column" is that row, the output the entry's CSR position. The launch
        // passes B as the staged operand and A as the gathered one; whole-plan launches only
        bool cols = false;
        DevBuf<u32> rowIds;
        // dynamic piece batches (k_sddmm_rb / k_sddmm_rb_pair<.., true>; Knobs::batches)
        bool dynBatches = false;
    };
    // rows of 128, 256, 512, 1024 and 2048 bytes, for fp32 [0, 5) and fp16/bf16 [5, 10) (tileMin)
    static constexpr int N_RB_SIZES = 5;
    static constexpr int N_RB_LAYOUTS = 2 * N_RB_SIZES;
    mutable RowBlockLayout rbl[N_RB_LAYOUTS];
    // whole-plan original-order candidates and, per slot, whether the launch uses it
    // (Knobs::orig_rows)
    mutable RowBlockLayout rblo[N_RB_LAYOUTS];
    mutable bool rb_use_orig[N_RB_LAYOUTS] = {};
    // whole-plan column-block layouts and whether the launch uses them (Knobs::col_blocks)
    mutable RowBlockLayout rblc[N_RB_LAYOUTS];
    mutable bool rb_use_cols[N_RB_LAYOUTS] = {};
    // layouts of panel ranges (row-panel shards, bsmr_sddmm_panels), most recent last
    static constexpr size_t MAX_SHARD_LAYOUTS = 16;
    // shared: a caller keeps its layout alive while another thread's request evicts it
    mutable std::vector<std::shared_ptr<RowBlockLayout>> shard_rbl;
    // layouts of panel ranges built through bsmr_plan_prepare_panels (oldest first, at most
    // MAX_SHARD_LAYOUTS): lazy builds never evict one; a further prepare drops the oldest
    mutable std::vector<std::shared_ptr<RowBlockLayout>> prep_rbl;
    int build_rowblock_layout(RowBlockLayout& L, u32 rowBytes, u32 pa, u32 pb, u32 tileMin,
                              bool orig = false, bool cols = false) const;
    // the whole plan's reordered-row layout of a row size (always built first; panel shards cut
    // its row blocks, and a local A follows its rows)
    const RowBlockLayout& rb_reordered(int slot, int dtype) const {
        return rbl[slot + (dtype != BSMR_F32 ? N_RB_SIZES : 0)];
    }
    // the whole-plan layout a launch of this slot uses (rbl, rblo or rblc)
    const RowBlockLayout& rb_whole(int slot) const {
        return rb_use_cols[slot] ? rblc[slot] : rb_use_orig[slot] ? rblo[slot] : rbl[slot];
    }
    // the (cached) layout for rows of rowBytes over panels [pa, pb) for fp32 (half = false) or
    // fp16/bf16 operands; null on error. Call with layout_mu held; the whole-plan layouts are
    // plan members (non-owning pointer), a shard layout is shared with the cache. keep: a panel
    // range's layout goes on (or moves to) the prepared list
    std::shared_ptr<const RowBlockLayout> rowblock_layout(u32 rowBytes, bool half, u32 pa, u32 pb,
                                                          int* err, bool keep = false) const;
    // the same lookup building nothing: null when a launch would have to build (layout_mu held)
    std::shared_ptr<const RowBlockLayout> rowblock_ready(u32 rowBytes, bool half, u32 pa,
                                                         u32 pb) const;
    // everything that depends on the column split is dropped (build_columns; layout_mu held)
    void drop_launch_layouts();

    mutable DevBuf<uint8_t> tmp;  // scan/sort scratch
    // BSMR_DIAG & 32 debug timeline (4 u64 per wave of the last launch)
    mutable DevBuf<unsigned long long> trace;
    mutable size_t traceN = 0;
    int prepare_trace(size_t waves, hipStream_t s) const {
        if (trace.size() < waves * 4) BSMR_CHECK(trace.alloc(waves * 4));
        BSMR_HIP(hipMemsetAsync(trace.data(), 0, waves * 4 * sizeof(unsigned long long), s));
        traceN = waves;
        return BSMR_OK;
    }
    mutable std::mutex layout_mu;
    // identity over reordered positions (built on first use): the row list of launches whose A
    // holds the shard's rows in reordered order (bsmr_sddmm_panels_local)
    mutable DevBuf<u32> iotaR;

    // dense-sampled launch: per 128 x 128 tile of P (original index space) its stored entries
    struct DenseLayout {
        bool built = false;
        u32 ntn = 0, ntiles = 0, nonempty = 0;
        DevBuf<u32> off, loc, out;  // loc = local row << 7 | local column; out = CSR position
    };
    mutable DenseLayout dense;
    int build_dense_layout() const;

    // panel-grouped tile launch (sddmm_half.hip k_sddmm_ptile): tile-dominated fp16/bf16 plans,
    // K in {64, 128, 256, 512}; items {panel, first tile, tiles <= tpi, 0} in launch order
    struct PtileLayout {
        bool built = false;
        u32 tpi = 0, nItems = 0, nListed = 0, waves = 8, stride = 0;
        // per item slot {first panel, first tile, tiles, second panel + 1 (0: one panel)}
        DevBuf<uint4> items;
        // per item slot (stride u32): 32 A rows (the first panel's 16, then the second's, or the
        // first's again), {first tile, tiles, tiles of the first panel, panels}, 12 zeros, 16
        // columns per tile (a block for every tile and at least one per wave)
        DevBuf<u32> desc;
        static u32 desc_waves(u32 tpi) { return tpi > 0 && tpi <= 4 ? 4u : 8u; }
        static u32 desc_stride(u32 tiles) { return 48 + 16 * tiles; }
    };
    mutable PtileLayout ptile;
    int build_ptile_layout(u32 tpi) const;
    bool ptile_ready() const { return ptile.built && ptile.tpi == k.ptile_tpi; }

    // plan-based SpMM (spmm.hip; bsmr_spmm / bsmr_spmm_t): one side's gather lists
    // (spmm_schedule.hpp: segments in launch order, sources, value positions, split
    // destinations) and the partial rows of its split destinations (partials x scratchK floats).
    // Built on first use or by bsmr_plan_prepare_spmm, under layout_mu; they depend on S and the
    // row order only, so build_columns keeps them
    struct SpmmSide {
        bool built = false;
        u32 chunk = 0, nSegs = 0, nReds = 0, splitDsts = 0, partials = 0, maxList = 0, scratchK = 0;
        DevBuf<SpmmSeg> segs;
        DevBuf<u32> src, vpos;
        DevBuf<SpmmRed> reds;
        DevBuf<float> scratch;
    };
    mutable SpmmSide spmm[2];  // [0] rows (bsmr_spmm), [1] columns (bsmr_spmm_t)

    // row softmax (softmax.hip; bsmr_softmax / bsmr_softmax_backward): the item list
    // (softmax_schedule.hpp), packed runs and wave rows apart from block rows. Built on first use
    // or by bsmr_plan_prepare_softmax, under layout_mu; it depends on rowptr only, so
    // build_columns keeps it
    struct SoftmaxList {
        bool built = false;
        u32 nRows = 0, nBlocks = 0, packedRuns = 0, waveRows = 0, maxRow = 0;
        DevBuf<SoftmaxItem> rows, blocks;
    };
    mutable SoftmaxList softmax;

    // fused sparse attention (attention.hip; bsmr_attention): the rows' segments of at most
    // ATTN_CHUNK entries (spmm_lists at side 1: src is colidx and vpos the identity, so neither is
    // kept), the split rows, and their partials: slices x partials x Dv accumulator rows followed by
    // slices x partials (m, l) pairs (bsmr_attention_heads; one slice for bsmr_attention); the
    // scratch holds what the largest slices x (Dv + 2) so far needs and never shrinks. Built on first use or by
    // bsmr_plan_prepare_attention / bsmr_plan_prepare_attention_heads, under
    // layout_mu; its own lists, which bsmr_plan_prepare_spmm never touches, and which depend on S
    // and the row order only, so build_columns keeps them
    struct AttentionState {
        bool built = false;
        u32 nSegs = 0, nReds = 0, splitRows = 0, partials = 0, maxRow = 0;
        DevBuf<SpmmSeg> segs;
        DevBuf<SpmmRed> reds;
        DevBuf<float> scratch;
    };
    mutable AttentionState attention;

    // fused sparse attention backward (attention_bwd.hip; bsmr_attention_backward): the rows'
    // segments (the forward's lists: AttentionState's buffers when they were built before this
    // state and the two chunks agree, rowShared, else lists of its own built the same way), the
    // columns' segments with the row of every entry (spmm_lists at side 2; no vpos: there are no
    // nnz values), and per slice (bsmr_attention_backward_heads; one for bsmr_attention_backward)
    // the M floats of delta = dot(GO, O) and the partial rows of the split destinations:
    // rowPartials x D floats, and colPartials x D followed by colPartials x Dv. Built
    // on first use or by bsmr_plan_prepare_attention_backward, under layout_mu; neither
    // bsmr_plan_prepare_spmm nor build_columns touches it, and it never writes AttentionState
    struct AttentionBwdState {
        bool built = false, rowShared = false;
        u32 rowSegs = 0, rowReds = 0, rowSplit = 0, rowPartials = 0, rowMax = 0;
        u32 colSegs = 0, colReds = 0, colSplit = 0, colPartials = 0, colMax = 0;
        DevBuf<SpmmSeg> rsegs, csegs;
        DevBuf<SpmmRed> rreds, creds;
        DevBuf<u32> csrc;
        DevBuf<float> delta, rowScratch, colScratch;  // the scratches hold what the largest (D, Dv) so far needs
        const SpmmSeg* row_segs(const AttentionState& f) const { return rowShared ? f.segs.data() : rsegs.data(); }
        const SpmmRed* row_reds(const AttentionState& f) const { return rowShared ? f.reds.data() : rreds.data(); }
    };
    mutable AttentionBwdState attention_bwd;

    int build_rows(const u32* h_rowptr, const u32* h_col);
    int build_columns();
    ~Plan() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// the whole plan's row-block layout for (K, dtype) (sddmm.hip); *out = null for column-major
int whole_rb_layout(const Plan& p, u32 K, int dtype, const Plan::RowBlockLayout** out,
                    bool reordered = false);

// ---- what launch_select.hpp reads from a plan ----
static_assert(LS_F32 == BSMR_F32 && LS_F16 == BSMR_F16 && LS_BF16 == BSMR_BF16 && LS_OK == BSMR_OK &&
                  LS_ERR_INVALID == BSMR_ERR_INVALID && LS_ERR_UNSUPPORTED == BSMR_ERR_UNSUPPORTED &&
                  LS_XCDS == XCD_BUCKETS,
              "launch_select.hpp constants");
inline PlanFacts launch_facts(const Plan& p) {
    return {p.M, p.N, p.nnz, p.nres, p.numDenseTiles};
}
inline LaunchChoice choose_launch(const Plan& p, u32 K, int dtype) {
    return choose_launch(launch_facts(p), p.k, K, dtype);
}
inline RbLayoutFacts rb_layout_facts(const Plan::RowBlockLayout& L) {
    return {L.rowBytes, L.NT, L.nItems, L.nTilesKept, L.outLds, L.outRuns, L.dynBatches};
}
// a rule's verdict as a status: its message goes to bsmr_last_error
inline int report(const Verdict& v) {
    if (v.code != BSMR_OK) set_error(v.msg);
    return v.code;
}

}  // namespace bsmr

struct bsmr_plan {
    bsmr::Plan p;
};
