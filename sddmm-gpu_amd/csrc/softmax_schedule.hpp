// softmax_schedule.hpp — host-only item list of the row softmax over the plan's pattern
// (bsmr_softmax / bsmr_softmax_backward). Standard library only: no HIP, no device, so it builds,
// runs and is sanitized on a machine without a GPU. softmax.hip downloads the plan's rowptr, calls
// softmax_items and uploads what it returns; bsmr_softmax_items (capi.cpp) is the same call over a
// caller's rowptr.
//
// A CSR row's entries are contiguous in P, so an item names rows and nothing else. Items are
// emitted in ascending row order; every non-empty row is in exactly one item:
//   packed run  kind = L (a power of two 1 .. 64): rows row .. row + count - 1, count <= 64 / L,
//               every non-empty one of ceil-power-of-two length L; lane group g (L lanes) of one
//               wave takes row + g, one entry per lane. Empty rows inside a run are idle groups;
//               a run never ends on an empty row;
//   wave row    kind = SOFTMAX_WAVE: one row of 64 < count <= SOFTMAX_WAVE_MAX entries, held in
//               the registers of one wave;
//   block row   kind = SOFTMAX_BLOCK: one row of count > SOFTMAX_WAVE_MAX entries, one workgroup,
//               in passes of SOFTMAX_BLOCK_PASS entries.
// `first` is rowptr[row]. How a row is summed depends on its length alone.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace bsmr {

constexpr uint32_t SOFTMAX_REGS = 16;                       // entries a lane holds
constexpr uint32_t SOFTMAX_WAVE_MAX = 64 * SOFTMAX_REGS;    // 1024
constexpr uint32_t SOFTMAX_BLOCK_WAVES = 16;                // waves of a block row's workgroup
constexpr uint32_t SOFTMAX_BLOCK_PASS = SOFTMAX_BLOCK_WAVES * SOFTMAX_WAVE_MAX;  // 16384
constexpr uint32_t SOFTMAX_WAVE = 0x100, SOFTMAX_BLOCK = 0x200;  // SoftmaxItem::kind beside L

// layout-compatible with bsmr_softmax_item (include/bsmr.h) and uint4
struct alignas(16) SoftmaxItem {
    uint32_t row, first, count, kind;
};

struct SoftmaxItems {
    std::vector<SoftmaxItem> items;  // ascending row
    uint64_t nItems = 0;             // also set by a count-only call
    uint32_t packedRuns = 0, waveRows = 0, blockRows = 0, maxRow = 0;
};

// 0 and `out` filled, or 1 (rowptr null or not non-decreasing from 0) and `err` naming the fault.
// count_only: the counts alone (no item is written).
int softmax_items(uint32_t M, const uint32_t* rowptr, SoftmaxItems& out, std::string& err,
                  bool count_only = false);

}  // namespace bsmr
