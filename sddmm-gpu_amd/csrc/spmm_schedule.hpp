// spmm_schedule.hpp — host-only gather lists of the plan-based SpMM (bsmr_spmm / bsmr_spmm_t, the
// gradients of bsmr_sddmm). Standard library only: no HIP, no device, so it builds, runs and is
// sanitized on a machine without a GPU. spmm.hip downloads the plan's CSR, calls spmm_lists and
// uploads what it returns; bsmr_spmm_lists (capi.cpp) is the same call over caller arrays.
//
// A side is rows (1: destination = row i, source = the entry's column, Y = S(V) B) or columns (2:
// destination = column j, source = the entry's row, Y = S(V)^T A). A destination's list holds its
// entries in ascending CSR position, whatever the column order inside a CSR row. Lists are stored
// destination after destination in ascending index (src / vpos, nnz each) and cut into segments
// of at most `chunk` entries, one wave each; a destination of several segments sums through
// consecutive partial slots, one per segment.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace bsmr {

constexpr uint32_t SPMM_DIRECT = 0xFFFFFFFFu;  // SpmmSeg::part of a segment that writes Y itself
// entries per segment unless the caller chooses: the fastest of {128, 256, 512, 1024} on the
// columns of the nips-like pattern (32.3 / 35.4 / 38.5 / 49.8 us), whose long
// lists otherwise leave a launch with too few waves
constexpr uint32_t SPMM_CHUNK_DEFAULT = 128;

// layout-compatible with bsmr_spmm_seg (include/bsmr.h) and uint4
struct alignas(16) SpmmSeg {
    uint32_t dst, first, count, part;
};
// a split destination: Y[dst] = partial[part0] + ... + partial[part0 + nparts - 1], in that order
struct alignas(16) SpmmRed {
    uint32_t dst, part0, nparts, pad;
};

struct SpmmIn {
    uint32_t M = 0, N = 0, nnz = 0;
    const uint32_t* rowptr = nullptr;  // M + 1
    const uint32_t* colidx = nullptr;  // nnz
    int side = 1;
    uint32_t chunk = SPMM_CHUNK_DEFAULT;
    // destinations in launch order (each at most once); the others follow in ascending index
    const uint32_t* order = nullptr;
    uint32_t norder = 0;
};

struct SpmmLists {
    std::vector<SpmmSeg> segs;  // launch order
    std::vector<uint32_t> src, vpos;
    std::vector<SpmmRed> reds;  // in the order their first segment is launched
    uint64_t nSegs = 0;         // also set by a count-only call
    uint32_t splitDsts = 0, partials = 0, maxList = 0, chunk = 0;
};

// 0 and `out` filled, or 1 (invalid input) and `err` naming the first fault. count_only: only
// out.nSegs, splitDsts, partials, maxList and chunk are set (no list is written).
int spmm_lists(const SpmmIn& in, SpmmLists& out, std::string& err, bool count_only = false);

}  // namespace bsmr
