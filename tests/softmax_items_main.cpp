// Stand-alone driver of the host-only softmax item list (csrc/softmax_schedule.cpp), built by
// tests/test_softmax_items_cpu.py under -fsanitize=address,undefined. Reads a pattern file ("M",
// then rowptr as decimal integers), builds the list, checks that it covers every non-empty row
// exactly once within the kinds' limits and prints "<items> <digest of the items>" for the test to
// compare with the library's answer.
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "softmax_schedule.hpp"

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <pattern file>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    uint32_t M;
    if (fscanf(f, "%" SCNu32, &M) != 1) return 2;
    std::vector<uint32_t> rp(static_cast<size_t>(M) + 1);
    for (uint32_t& x : rp)
        if (fscanf(f, "%" SCNu32, &x) != 1) return 2;
    fclose(f);
    bsmr::SoftmaxItems L, C;
    std::string err;
    if (bsmr::softmax_items(M, rp.data(), L, err) || bsmr::softmax_items(M, rp.data(), C, err, true)) {
        printf("invalid: %s\n", err.c_str());
        return 1;
    }
    std::vector<uint8_t> seen(M, 0);
    uint32_t next = 0;
    for (const bsmr::SoftmaxItem& it : L.items) {
        if (it.row < next || it.row >= M || it.first != rp[it.row]) return 3;
        const bool packed = it.kind <= 64;
        const uint32_t rows = packed ? it.count : 1;
        if (packed && (it.kind == 0 || (it.kind & (it.kind - 1)) || it.count == 0 || it.count > 64 / it.kind)) return 3;
        if (static_cast<uint64_t>(it.row) + rows > M) return 3;
        for (uint32_t r = it.row; r < it.row + rows; ++r) {
            const uint32_t n = rp[r + 1] - rp[r];
            if (seen[r]++) return 3;
            if (packed ? n > it.kind : n != it.count) return 3;
        }
        if (it.kind == bsmr::SOFTMAX_WAVE && (it.count <= 64 || it.count > bsmr::SOFTMAX_WAVE_MAX)) return 3;
        if (it.kind == bsmr::SOFTMAX_BLOCK && it.count <= bsmr::SOFTMAX_WAVE_MAX) return 3;
        if (!packed && it.kind != bsmr::SOFTMAX_WAVE && it.kind != bsmr::SOFTMAX_BLOCK) return 3;
        next = it.row + rows;
    }
    for (uint32_t r = 0; r < M; ++r)
        if (!seen[r] && rp[r + 1] != rp[r]) return 3;
    if (L.items.size() != L.nItems || C.nItems != L.nItems || !C.items.empty() || C.packedRuns != L.packedRuns ||
        C.waveRows != L.waveRows || C.blockRows != L.blockRows || C.maxRow != L.maxRow ||
        L.packedRuns + L.waveRows + L.blockRows != L.nItems)
        return 3;
    // digest: sum over the words x_i of (x_i + 1)(2 i + 1) c, modulo 2^64
    uint64_t h = 0, i = 0;
    for (const bsmr::SoftmaxItem& it : L.items) {
        const uint32_t w[4] = {it.row, it.first, it.count, it.kind};
        for (uint32_t x : w) h += (static_cast<uint64_t>(x) + 1) * (2 * i++ + 1) * 0x9E3779B97F4A7C15ull;
    }
    printf("%" PRIu64 " %016" PRIx64 "\n", L.nItems, h);
    return 0;
}
