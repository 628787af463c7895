// attention_panels.hpp — host-only lists of the panel form of the fused sparse attention forward
// (bsmr_attention_panels, attention_panels.hip). Standard library only: no HIP, no device, so it
// builds, runs and is sanitized on a machine without a GPU. attention_panels.hip downloads the
// plan's CSR and row order, calls attention_panel_lists and uploads what it returns;
// bsmr_attention_panel_lists (capi.cpp) is the same call over caller arrays.
//
// A panel is PANEL_ROWS consecutive rows of the launch order (the caller's order, then every row it
// does not name in ascending index: those rows get trailing panels of their own and are computed like
// any other, so every row of the matrix is written whether or not the unnamed rows are empty); the last panel may be short. Per panel the ascending union of its rows'
// columns is cut into steps of PANEL_STEP_COLS columns: a step holds the columns and, per panel
// row, a mask whose bit c says that the row stores cols[c]. The padding slots of a panel's last
// step repeat the step's first column with mask bit 0 in every row: a load of a padding slot stays
// in bounds and brings in nothing that the panel does not reference. An item is at most
// PANEL_ITEM_STEPS consecutive steps of one panel, one wave; a panel of several items sums
// through consecutive partial slots, one per item (16 rows each), and has an entry in the reduce
// list. A panel whose rows are all empty is one item of 0 steps.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace bsmr {

constexpr uint32_t PANEL_ROWS = 16;
constexpr uint32_t PANEL_STEP_COLS = 32;
// steps per item: 512 union columns. A wave keeps its Q registers for the whole item, and a
// 16 x 16 block mask row of up to 32 blocks stays one item (no partials, no reduce launch)
constexpr uint32_t PANEL_ITEM_STEPS = 16;
constexpr uint32_t PANEL_DIRECT = 0xFFFFFFFFu;  // PanelItem::part of an item that writes O itself

// layout-compatible with bsmr_attention_panel_step / _item / _red (include/bsmr.h)
struct alignas(64) PanelStep {
    uint32_t cols[PANEL_STEP_COLS];
    uint32_t masks[PANEL_ROWS];
};
// rows[row0 .. row0 + min(16, M - row0)) of the launch order; steps[step0 .. step0 + nsteps)
struct alignas(16) PanelItem {
    uint32_t row0, step0, nsteps, part;
};
// a split panel: partial slots part0 .. part0 + nparts - 1, in item order
struct alignas(16) PanelRed {
    uint32_t row0, part0, nparts, pad;
};

struct PanelLists {
    std::vector<uint32_t> rows;  // the launch order, M entries
    std::vector<PanelStep> steps;
    std::vector<PanelItem> items;  // launch order: panel after panel, a panel's items in step order
    std::vector<PanelRed> reds;
    uint64_t nSteps = 0, nItems = 0;
    uint32_t panels = 0, splitPanels = 0, partials = 0;
};

// 0 and `out` filled; 1 for invalid input (rowptr not ascending from 0, a column >= N, a column
// twice in a row, an order entry >= M or twice); 2 for a pattern past the lists' capacity (more than
// 2^32 - 1 steps, items or partials); `err` names the first fault.
int attention_panel_lists(uint32_t M, uint32_t N, const uint32_t* rowptr, const uint32_t* colidx, const uint32_t* order,
                          uint32_t norder, PanelLists& out, std::string& err);

// The pattern of S^T as a CSR of N rows (trowptr: N + 1 entries; tcolidx: row j holds the rows that
// store column j, ascending): the panel backward's columns side is attention_panel_lists on it with
// M and N swapped and an empty order, so a column panel is 16 consecutive columns. 0, or 1 with
// `err` set for a rowptr not ascending from 0 or a column >= N.
int attention_pattern_transpose(uint32_t M, uint32_t N, const uint32_t* rowptr, const uint32_t* colidx,
                                std::vector<uint32_t>& trowptr, std::vector<uint32_t>& tcolidx, std::string& err);

// 1000 nnz / (16 x 32 x steps): how full the steps' masks are (0 without steps)
inline uint32_t panel_fill_permille(uint64_t nnz, uint64_t steps) {
    return steps ? static_cast<uint32_t>(1000u * nnz / (PANEL_ROWS * PANEL_STEP_COLS * steps)) : 0u;
}

}  // namespace bsmr
