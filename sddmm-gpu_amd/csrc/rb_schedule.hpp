// rb_schedule.hpp — the host-only part of the row-block launch layout: block geometry
// (rb_geometry), item scheduling (rb_schedule) and the run table of staged output (rb_cut_runs).
// Standard library and knobs.hpp only: no HIP, no device, so it builds, runs and is tested on a
// machine without a GPU. plan.hip (Plan::build_rowblock_layout) sorts the entries on the device,
// calls these, and uploads what they return.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <thread>
#include <vector>

#include "knobs.hpp"

namespace bsmr {

constexpr uint32_t RB_XCDS = 8;                    // XCD_BUCKETS (plan.hpp)
constexpr uint32_t RB_COL_MASK = (1u << 22) - 1;   // the column of a sorted entry word

// an item {row block, kept-tile begin, kept-tile end, piece begin}: layout-compatible with uint4
struct alignas(16) RbItem {
    uint32_t x, y, z, w;
};
// a piece {first entry, column | (length - 1) << 22}, or an item's {first entry, entries}:
// layout-compatible with uint2
struct alignas(8) RbPiece {
    uint32_t x, y;
};

struct RbGeometry {
    uint32_t rowBytes = 0;
    bool orig = false, cols = false;  // original-order row blocks / column blocks (whole plan)
    uint32_t RB = 0, NT = 0, nRB = 0;  // rows per block, threads per workgroup, blocks
    size_t lds = 0;                    // the A image: RB * rowBytes
    uint32_t l2Kb = 0, m = 1;          // column-range budget; ranges per XCD
    bool stagedWanted = false, staged = false;
    uint32_t outCap = 0;     // results the LDS past the image holds
    uint32_t perBucket = 1;  // workgroup slots per XCD
};

// Rows per row block for rows of rowBytes: a multiple of 16 with RB * rowBytes within the LDS
// budget, at most 1024 (10-bit local row in the entry metadata) and no more than the matrix needs.
uint32_t rowblock_rows(uint32_t rowBytes, uint32_t lds_kb, uint32_t R);

// Block geometry of a layout over Rs staged rows holding n0 entries (before tile demotion), the
// gathered index space of NS columns, on a device of cus compute units; nnz = the plan's.
RbGeometry rb_geometry(uint32_t rowBytes, uint32_t Rs, uint32_t n0, uint32_t NS, uint32_t nnz, int cus,
                       bool orig, bool cols, const Knobs& k);

struct RbScheduleIn {
    // the entries sorted by (row block, column): words whose low 22 bits are the column (read in
    // place, never copied)
    const uint32_t* entries = nullptr;
    size_t n = 0;
    const uint32_t* rbEnd = nullptr;  // per row block: end of its entries (non-decreasing)
    // kept tiles of row block b: positions [keptBegin[b], keptBegin[b + 1]) of the kept list
    // (nRB + 1 values); null: no kept tiles
    const uint32_t* keptBegin = nullptr;
    uint32_t NS = 0;
    RbGeometry geom;
    const Knobs* knobs = nullptr;  // the plan's tuning (Plan::k); read in place
    unsigned threads = 0;  // host threads (0: up to 16); the result does not depend on it
    std::function<void(const char*)> lap;  // called after each phase with its name (may be empty)
};

struct RbScheduleOut {
    std::vector<RbItem> items;    // launch order: list position j of XCD x at j * 8 + x
    std::vector<uint32_t> ends;   // per item: piece end
    std::vector<RbPiece> pieces;
    std::vector<RbPiece> ient;    // per item {first entry, entries}
    std::vector<RbItem> itemStat;  // per item {row block, kept tiles, entries, pieces}; padding 0
    std::vector<double> rbCost;   // per row block: the shard cost model
    uint32_t nWorkItems = 0;
    bool dyn = false;  // dynamic piece batches
};

// Items, pieces and statistics of a layout from its sorted entries. Never touches a device.
void rb_schedule(const RbScheduleIn& in, RbScheduleOut& out);

// Run table of staged output (plan.hpp RowBlockLayout::outRuns): an item's slots are its entries
// sorted by CSR position; up to RB_RUN_MAX consecutive positions form one run {first position,
// first slot | length << 16}: one wave store (an unsplit original-order item is one long run,
// which would leave all but one wave idle in the store pass, hence the cut). The table is used
// when no item has more runs than the workgroup has lanes (one descriptor per lane); else the
// layout keeps the per-result positions.
constexpr uint32_t RB_RUN_MAX = 64;

struct RbRuns {
    bool fits = false;              // every item has at most NT runs
    std::vector<RbPiece> itemRuns;  // per item {first run, runs} (the counts also when !fits)
    std::vector<RbPiece> runs;      // the flat table in item order; empty when !fits
};

// sortedPos: every item's positions in ascending order at [ient[i].x, + ient[i].y) (slots below
// 65536 per item: the caller's outCap). Never touches a device; the result does not depend on
// `threads` (0: up to 16).
void rb_cut_runs(const uint32_t* sortedPos, const RbPiece* ient, size_t nItems, uint32_t NT, RbRuns& out,
                 unsigned threads = 0);

// f(thread, begin, end) over [0, n) on up to `threads` host threads (0: up to 16): contiguous
// ranges, each index visited once (results written per index are independent of the split)
template <class F>
void par_for(size_t n, F&& f, size_t serial_below = 2048, unsigned threads = 0) {
    const unsigned T = threads ? threads : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (n < serial_below || T == 1) {
        f(0u, size_t{0}, n);
        return;
    }
    std::vector<std::thread> th;
    const size_t chunk = (n + T - 1) / T;
    for (unsigned t = 0; t < T; ++t) {
        const size_t a = t * chunk, b = std::min(n, a + chunk);
        if (a < b) th.emplace_back([&f, t, a, b]() { f(t, a, b); });
    }
    for (auto& x : th) x.join();
}

}  // namespace bsmr
