// Stand-alone driver of the host-only SpMM gather lists (csrc/spmm_schedule.cpp), built by
// tests/test_spmm_lists_cpu.py under -fsanitize=address,undefined. Reads a pattern file
// ("M N nnz norder", then rowptr, colidx and order as decimal integers), builds the lists of
// (side, chunk), checks them against the pattern and prints "<segments> <digest of segs, src,
// vpos>" for the test to compare with the library's answer.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "spmm_schedule.hpp"

static bool read_u32(FILE* f, std::vector<uint32_t>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (fscanf(f, "%" SCNu32, &v[i]) != 1) return false;
    return true;
}

// digest: sum over the words x_i of (x_i + 1)(2 i + 1) c, modulo 2^64 (i counts across calls)
static void digest(uint64_t& h, uint64_t& i, const uint32_t* p, size_t n) {
    for (size_t k = 0; k < n; ++k, ++i) h += (static_cast<uint64_t>(p[k]) + 1) * (2 * i + 1) * 0x9E3779B97F4A7C15ull;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s <pattern file> <side> <chunk>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    uint32_t M, N, nnz, norder;
    std::vector<uint32_t> rp, ci, order;
    if (fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &M, &N, &nnz, &norder) != 4 ||
        !read_u32(f, rp, static_cast<size_t>(M) + 1) || !read_u32(f, ci, nnz) || !read_u32(f, order, norder)) {
        fprintf(stderr, "bad pattern file\n");
        return 2;
    }
    fclose(f);
    bsmr::SpmmIn in;
    in.M = M;
    in.N = N;
    in.nnz = nnz;
    in.rowptr = rp.data();
    in.colidx = ci.data();
    in.side = atoi(argv[2]);
    in.chunk = static_cast<uint32_t>(strtoul(argv[3], nullptr, 10));
    in.order = norder ? order.data() : nullptr;
    in.norder = norder;
    bsmr::SpmmLists L, C;
    std::string err;
    if (bsmr::spmm_lists(in, L, err) || bsmr::spmm_lists(in, C, err, true)) {
        printf("invalid: %s\n", err.c_str());
        return 1;
    }
    // every stored entry once, no segment over the chunk, the count-only call agrees
    std::vector<uint8_t> seen(nnz, 0);
    uint32_t parts = 0;
    for (const bsmr::SpmmSeg& s : L.segs) {
        if (s.count > in.chunk || static_cast<uint64_t>(s.first) + s.count > nnz) return 3;
        for (uint32_t e = s.first; e < s.first + s.count; ++e) {
            if (L.vpos[e] >= nnz || seen[L.vpos[e]]++) return 3;
            const uint32_t other = in.side == 1 ? ci[L.vpos[e]] : s.dst;
            if (other != (in.side == 1 ? L.src[e] : ci[L.vpos[e]])) return 3;
        }
        parts += s.part != bsmr::SPMM_DIRECT;
    }
    for (uint32_t e = 0; e < nnz; ++e)
        if (!seen[e]) return 3;
    uint32_t redParts = 0;
    for (const bsmr::SpmmRed& r : L.reds) redParts += r.nparts;
    if (parts != L.partials || redParts != parts || L.segs.size() != L.nSegs || C.nSegs != L.nSegs ||
        C.partials != L.partials || C.maxList != L.maxList || C.splitDsts != L.reds.size())
        return 3;
    uint64_t h = 0, i = 0;
    for (const bsmr::SpmmSeg& s : L.segs) {
        const uint32_t w[4] = {s.dst, s.first, s.count, s.part};
        digest(h, i, w, 4);
    }
    digest(h, i, L.src.data(), L.src.size());
    digest(h, i, L.vpos.data(), L.vpos.size());
    printf("%" PRIu64 " %016" PRIx64 "\n", L.nSegs, h);
    return 0;
}
