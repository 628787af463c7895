// attention_panels.cpp — panel lists of the fused sparse attention forward on matrix instructions
// (attention_panels.hpp). Plain C++.
#include "attention_panels.hpp"

#include <algorithm>

namespace bsmr {

int attention_panel_lists(uint32_t M, uint32_t N, const uint32_t* rowptr, const uint32_t* colidx, const uint32_t* order,
                          uint32_t norder, PanelLists& out, std::string& err) {
    out = PanelLists{};
    if (!rowptr) {
        err = "null rowptr";
        return 1;
    }
    if (rowptr[0] != 0) {
        err = "rowptr[0] != 0";
        return 1;
    }
    for (uint32_t r = 0; r < M; ++r)
        if (rowptr[r + 1] < rowptr[r]) {
            err = "rowptr is not non-decreasing at row " + std::to_string(r);
            return 1;
        }
    if (M && rowptr[M] && !colidx) {
        err = "null colidx";
        return 1;
    }
    if (norder && !order) {
        err = "null order";
        return 1;
    }
    // the launch order: the caller's rows, then the rows it does not name in ascending index. Those
    // rows are computed like any other (an empty one gives O = 0 and LSE = -inf): nothing here or
    // in the kernel relies on their being empty
    std::vector<uint32_t> rows;
    rows.reserve(M);
    std::vector<bool> named(M, false);
    for (uint32_t i = 0; i < norder; ++i) {
        if (order[i] >= M || named[order[i]]) {
            err = "order entry " + std::to_string(i) + (order[i] >= M ? " is not a row" : " names a row twice");
            return 1;
        }
        named[order[i]] = true;
        rows.push_back(order[i]);
    }
    for (uint32_t r = 0; r < M; ++r)
        if (!named[r]) rows.push_back(r);

    std::vector<uint32_t> uni;
    uint64_t partials = 0;
    for (uint32_t row0 = 0; row0 < M; row0 += PANEL_ROWS) {
        const uint32_t nrows = std::min(PANEL_ROWS, M - row0);
        uni.clear();
        for (uint32_t r = 0; r < nrows; ++r) {
            const uint32_t row = rows[row0 + r];
            for (uint32_t e = rowptr[row]; e < rowptr[row + 1]; ++e) {
                if (colidx[e] >= N) {
                    err = "column " + std::to_string(colidx[e]) + " of row " + std::to_string(row) + " is not below N";
                    return 1;
                }
                uni.push_back(colidx[e]);
            }
        }
        std::sort(uni.begin(), uni.end());
        uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
        const uint64_t nsteps = (uni.size() + PANEL_STEP_COLS - 1) / PANEL_STEP_COLS;
        const uint64_t step0 = out.nSteps;
        const uint64_t nitems = std::max<uint64_t>(1, (nsteps + PANEL_ITEM_STEPS - 1) / PANEL_ITEM_STEPS);
        if (step0 + nsteps > 0xFFFFFFFFull || out.nItems + nitems > 0xFFFFFFFFull || partials + nitems > 0xFFFFFFFFull) {
            err = "more than 2^32 - 1 steps, items or partials";
            return 2;
        }
        ++out.panels;
        out.nSteps += nsteps;
        out.nItems += nitems;
        if (nitems > 1) {
            ++out.splitPanels;
            out.reds.push_back({row0, static_cast<uint32_t>(partials), static_cast<uint32_t>(nitems), 0u});
        }
        for (uint64_t i = 0; i < nitems; ++i) {
            const uint64_t s0 = i * PANEL_ITEM_STEPS;
            out.items.push_back({row0, static_cast<uint32_t>(step0 + s0),
                                 static_cast<uint32_t>(std::min<uint64_t>(PANEL_ITEM_STEPS, nsteps - std::min(nsteps, s0))),
                                 nitems > 1 ? static_cast<uint32_t>(partials + i) : PANEL_DIRECT});
        }
        out.steps.resize(step0 + nsteps);  // (masks 0)
        for (size_t u = 0; u < nsteps * PANEL_STEP_COLS; ++u) {
            PanelStep& st = out.steps[step0 + u / PANEL_STEP_COLS];
            st.cols[u % PANEL_STEP_COLS] = u < uni.size() ? uni[u] : st.cols[0];
        }
        // the rows' bits; a column twice in a row cannot be a mask bit
        for (uint32_t r = 0; r < nrows; ++r) {
            const uint32_t row = rows[row0 + r];
            uint64_t bits = 0;
            for (uint32_t e = rowptr[row]; e < rowptr[row + 1]; ++e) {
                const size_t u = static_cast<size_t>(std::lower_bound(uni.begin(), uni.end(), colidx[e]) - uni.begin());
                uint32_t& mask = out.steps[step0 + u / PANEL_STEP_COLS].masks[r];
                bits += !((mask >> (u % PANEL_STEP_COLS)) & 1u);
                mask |= 1u << (u % PANEL_STEP_COLS);
            }
            if (bits != rowptr[row + 1] - rowptr[row]) {
                err = "row " + std::to_string(row) + " stores a column twice";
                return 1;
            }
        }
        if (nitems > 1) partials += nitems;
    }
    out.partials = static_cast<uint32_t>(partials);
    out.rows = std::move(rows);
    return 0;
}

int attention_pattern_transpose(uint32_t M, uint32_t N, const uint32_t* rowptr, const uint32_t* colidx,
                                std::vector<uint32_t>& trowptr, std::vector<uint32_t>& tcolidx, std::string& err) {
    trowptr.assign(static_cast<size_t>(N) + 1, 0u);
    tcolidx.clear();
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
    if (nnz && !colidx) {
        err = "null colidx";
        return 1;
    }
    for (uint32_t e = 0; e < nnz; ++e) {
        if (colidx[e] >= N) {
            err = "column " + std::to_string(colidx[e]) + " is not below N";
            return 1;
        }
        ++trowptr[colidx[e] + 1];
    }
    for (uint32_t j = 0; j < N; ++j) trowptr[j + 1] += trowptr[j];
    // rows in ascending order: a column's rows come out ascending
    tcolidx.resize(nnz);
    std::vector<uint32_t> next(trowptr.begin(), trowptr.end() - 1);
    for (uint32_t r = 0; r < M; ++r)
        for (uint32_t e = rowptr[r]; e < rowptr[r + 1]; ++e) tcolidx[next[colidx[e]]++] = r;
    return 0;
}

}  // namespace bsmr
