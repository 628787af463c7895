// spmm_panels.cpp — entry positions of the panel form of SpMM (spmm_panels.hpp). Plain C++.
#include "spmm_panels.hpp"

#include <algorithm>
#include <utility>

namespace bsmr {

int spmm_pattern_transpose_pos(uint32_t M, uint32_t N, const uint32_t* rowptr, const uint32_t* colidx,
                               std::vector<uint32_t>& trowptr, std::vector<uint32_t>& tcolidx, std::vector<uint32_t>& tpos,
                               std::string& err) {
    tpos.clear();
    if (const int st = attention_pattern_transpose(M, N, rowptr, colidx, trowptr, tcolidx, err)) return st;
    // the same fill as the transpose: rows ascending, so entry k of column j is the k-th row that stores j
    tpos.resize(tcolidx.size());
    std::vector<uint32_t> next(trowptr.begin(), trowptr.end() - 1);
    for (uint32_t r = 0; r < M; ++r)
        for (uint32_t e = rowptr[r]; e < rowptr[r + 1]; ++e) tpos[next[colidx[e]]++] = e;
    return 0;
}

int spmm_panel_positions(uint32_t M, uint32_t N, const uint32_t* rowptr, const uint32_t* colidx, const uint32_t* epos,
                         const uint32_t* rows, const PanelStep* steps, uint64_t nsteps, const PanelItem* items, uint64_t nitems,
                         std::vector<uint32_t>& base, std::vector<uint32_t>& pos, std::string& err) {
    base.clear();
    pos.clear();
    if (!rowptr || rowptr[0] != 0) {
        err = "rowptr is null or rowptr[0] != 0";
        return 1;
    }
    for (uint32_t r = 0; r < M; ++r)
        if (rowptr[r + 1] < rowptr[r]) {
            err = "rowptr is not non-decreasing at row " + std::to_string(r);
            return 1;
        }
    const uint32_t nnz = rowptr[M];
    if ((nnz && !colidx) || (M && !rows) || (nsteps && !steps) || (nitems && !items)) {
        err = "null colidx, rows, steps or items";
        return 1;
    }
    base.assign(static_cast<size_t>(PANEL_ROWS) * nsteps, 0u);
    pos.reserve(nnz);
    // a panel row's entries by column, and how many of them the panel's steps have taken so far
    std::vector<std::pair<uint32_t, uint32_t>> ent[PANEL_ROWS];
    size_t taken[PANEL_ROWS] = {};
    uint32_t nrows = 0;
    auto all_taken = [&]() {
        for (uint32_t r = 0; r < nrows; ++r)
            if (taken[r] != ent[r].size()) return false;
        return true;
    };
    for (uint64_t i = 0; i < nitems; ++i) {
        const PanelItem& it = items[i];
        if (it.row0 >= M || it.step0 > nsteps || it.nsteps > nsteps - it.step0) {
            err = "item " + std::to_string(i) + " is out of range";
            return 1;
        }
        if (i == 0 || it.row0 != items[i - 1].row0) {  // a new panel
            if (!all_taken()) break;
            nrows = std::min(PANEL_ROWS, M - it.row0);
            for (uint32_t r = 0; r < nrows; ++r) {
                const uint32_t row = rows[it.row0 + r];
                if (row >= M) {
                    err = "rows entry " + std::to_string(it.row0 + r) + " is not a row";
                    return 1;
                }
                ent[r].clear();
                taken[r] = 0;
                for (uint32_t e = rowptr[row]; e < rowptr[row + 1]; ++e) ent[r].emplace_back(colidx[e], e);
                std::sort(ent[r].begin(), ent[r].end());
            }
        }
        for (uint64_t s = it.step0; s < static_cast<uint64_t>(it.step0) + it.nsteps; ++s)
            for (uint32_t r = 0; r < PANEL_ROWS; ++r) {
                base[PANEL_ROWS * s + r] = static_cast<uint32_t>(pos.size());
                for (uint32_t mask = steps[s].masks[r]; mask; mask &= mask - 1) {
                    const uint32_t col = steps[s].cols[__builtin_ctz(mask)];
                    if (r >= nrows || taken[r] == ent[r].size() || ent[r][taken[r]].first != col || col >= N || pos.size() == nnz) {
                        err = "step " + std::to_string(s) + ", row " + std::to_string(r) + ": the pattern does not store column " +
                              std::to_string(col) + " there (lists of another pattern)";
                        return 1;
                    }
                    const uint32_t e = ent[r][taken[r]++].second;
                    pos.push_back(epos ? epos[e] : e);
                }
            }
    }
    if (!all_taken() || pos.size() != nnz) {
        err = "the lists do not hold every stored entry exactly once";
        return 1;
    }
    return 0;
}

}  // namespace bsmr
