// softmax_schedule.cpp — item list of the row softmax (softmax_schedule.hpp). Plain C++.
#include "softmax_schedule.hpp"

#include <algorithm>

namespace bsmr {

namespace {

// the packed class of a row of 1 .. 64 entries: the next power of two
uint32_t lane_class(uint32_t len) {
    uint32_t L = 1;
    while (L < len) L <<= 1;
    return L;
}

}  // namespace

int softmax_items(uint32_t M, const uint32_t* rowptr, SoftmaxItems& out, std::string& err, bool count_only) {
    out = SoftmaxItems{};
    if (!rowptr) {
        err = "null rowptr";
        return 1;
    }
    if (rowptr[0] != 0) {
        err = "rowptr[0] != 0";
        return 1;
    }
    for (uint32_t r = 0; r < M; ++r) {
        if (rowptr[r + 1] < rowptr[r]) {
            err = "rowptr is not non-decreasing at row " + std::to_string(r);
            return 1;
        }
        out.maxRow = std::max(out.maxRow, rowptr[r + 1] - rowptr[r]);
    }
    auto len = [&](uint32_t r) { return rowptr[r + 1] - rowptr[r]; };
    auto emit = [&](uint32_t row, uint32_t count, uint32_t kind) {
        ++out.nItems;
        if (!count_only) out.items.push_back({row, rowptr[row], count, kind});
    };
    uint32_t r = 0;
    while (r < M) {
        const uint32_t n = len(r);
        if (n == 0) {
            ++r;
        } else if (n > SOFTMAX_WAVE_MAX) {
            ++out.blockRows;
            emit(r++, n, SOFTMAX_BLOCK);
        } else if (n > 64) {
            ++out.waveRows;
            emit(r++, n, SOFTMAX_WAVE);
        } else {
            // greedy run: grows while the next row is empty (an idle group) or of the same class
            // and a lane group is free; trailing empty rows are left out
            const uint32_t L = lane_class(n), groups = 64 / L;
            uint32_t last = r;
            for (uint32_t q = r + 1; q < M && q - r < groups; ++q) {
                const uint32_t nq = len(q);
                if (nq == 0) continue;
                if (nq > 64 || lane_class(nq) != L) break;
                last = q;
            }
            ++out.packedRuns;
            emit(r, last - r + 1, L);
            r = last + 1;
        }
    }
    return 0;
}

}  // namespace bsmr
