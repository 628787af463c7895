// spmm_schedule.cpp — gather lists of the plan-based SpMM (spmm_schedule.hpp). Plain C++.
#include "spmm_schedule.hpp"

#include <algorithm>

namespace bsmr {

namespace {

int fail(std::string& err, const std::string& msg) {
    err = msg;
    return 1;
}

}  // namespace

int spmm_lists(const SpmmIn& in, SpmmLists& out, std::string& err, bool count_only) {
    const uint32_t M = in.M, N = in.N, nnz = in.nnz;
    if (in.chunk == 0) return fail(err, "chunk must be >= 1");
    if (in.side != 1 && in.side != 2) return fail(err, "side must be 1 (rows) or 2 (columns)");
    if (!in.rowptr || (nnz && !in.colidx) || (in.norder && !in.order))
        return fail(err, "null array");
    if (in.rowptr[0] != 0) return fail(err, "rowptr[0] != 0");
    for (uint32_t r = 0; r < M; ++r)
        if (in.rowptr[r + 1] < in.rowptr[r] || in.rowptr[r + 1] > nnz)
            return fail(err, "rowptr is not non-decreasing within [0, nnz] at row " + std::to_string(r));
    if (in.rowptr[M] != nnz) return fail(err, "rowptr[M] != nnz");
    for (uint32_t e = 0; e < nnz; ++e)
        if (in.colidx[e] >= N)
            return fail(err, "colidx[" + std::to_string(e) + "] = " + std::to_string(in.colidx[e]) +
                                 " is not below N = " + std::to_string(N));
    const uint32_t D = in.side == 1 ? M : N;  // destinations
    std::vector<char> listed(D, 0);
    for (uint32_t q = 0; q < in.norder; ++q) {
        const uint32_t d = in.order[q];
        if (d >= D) return fail(err, "order[" + std::to_string(q) + "] = " + std::to_string(d) +
                                         " is not a destination (" + std::to_string(D) + ")");
        if (listed[d]) return fail(err, "order lists destination " + std::to_string(d) + " twice");
        listed[d] = 1;
    }

    // list offsets per destination (ascending index): the CSR's own for rows, a count for columns
    std::vector<uint32_t> off(static_cast<size_t>(D) + 1, 0);
    if (in.side == 1) {
        std::copy(in.rowptr, in.rowptr + M + 1, off.begin());
    } else {
        for (uint32_t e = 0; e < nnz; ++e) ++off[in.colidx[e] + 1];
        for (uint32_t d = 0; d < D; ++d) off[d + 1] += off[d];
    }

    const uint32_t chunk = in.chunk;
    out = SpmmLists{};
    out.chunk = chunk;
    auto nseg = [&](uint32_t d) -> uint32_t {
        const uint32_t len = off[d + 1] - off[d];
        return len == 0 ? 1u : (len - 1) / chunk + 1;
    };
    for (uint32_t d = 0; d < D; ++d) {
        const uint32_t len = off[d + 1] - off[d], ns = nseg(d);
        out.nSegs += ns;
        out.maxList = std::max(out.maxList, len);
        if (ns > 1) {
            ++out.splitDsts;
            out.partials += ns;
        }
    }
    if (count_only) return 0;

    out.src.resize(nnz);
    out.vpos.resize(nnz);
    if (in.side == 1) {
        for (uint32_t e = 0; e < nnz; ++e) {
            out.src[e] = in.colidx[e];
            out.vpos[e] = e;
        }
    } else {
        // stable counting sort by column: CSR positions ascend inside a column's list
        std::vector<uint32_t> fill(off.begin(), off.end() - 1);
        for (uint32_t r = 0; r < M; ++r)
            for (uint32_t e = in.rowptr[r]; e < in.rowptr[r + 1]; ++e) {
                const uint32_t k = fill[in.colidx[e]]++;
                out.src[k] = r;
                out.vpos[k] = e;
            }
    }

    out.segs.reserve(out.nSegs);
    out.reds.reserve(out.splitDsts);
    uint32_t part = 0;
    auto emit = [&](uint32_t d) {
        const uint32_t a = off[d], len = off[d + 1] - off[d], ns = nseg(d);
        if (ns == 1) {
            out.segs.push_back({d, a, len, SPMM_DIRECT});
            return;
        }
        out.reds.push_back({d, part, ns, 0});
        for (uint32_t s = 0; s < ns; ++s)
            out.segs.push_back({d, a + s * chunk, std::min(chunk, len - s * chunk), part++});
    };
    for (uint32_t q = 0; q < in.norder; ++q) emit(in.order[q]);
    for (uint32_t d = 0; d < D; ++d)
        if (!listed[d]) emit(d);
    return 0;
}

}  // namespace bsmr
