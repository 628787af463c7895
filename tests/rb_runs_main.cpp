// Stand-alone driver of the host-only run cutting (csrc/rb_schedule.cpp rb_cut_runs) for sanitizer
// builds: tests/test_store_ref_cpu.py compiles it with -fsanitize=address,undefined and compares
// its output with the library's. Input file: NT, threads, n items, then n pairs {first entry,
// entries}, then the sorted positions. Output: fits, runs, and the FNV-1a hash of the itemRuns
// words followed by the run words.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rb_schedule.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    unsigned NT = 0, threads = 0;
    unsigned long long n = 0;
    if (std::fscanf(f, "%u %u %llu", &NT, &threads, &n) != 3) return 2;
    std::vector<bsmr::RbPiece> ient(n);
    unsigned long long npos = 0;
    for (auto& e : ient) {
        if (std::fscanf(f, "%u %u", &e.x, &e.y) != 2) return 2;
        npos = npos > static_cast<unsigned long long>(e.x) + e.y ? npos : static_cast<unsigned long long>(e.x) + e.y;
    }
    std::vector<uint32_t> pos(npos);
    for (auto& p : pos)
        if (std::fscanf(f, "%u", &p) != 1) return 2;
    std::fclose(f);
    bsmr::RbRuns rr;
    bsmr::rb_cut_runs(pos.data(), ient.data(), ient.size(), NT, rr, threads);
    uint64_t h = 0xcbf29ce484222325ull;
    const auto mix = [&](uint32_t w) {
        for (int b = 0; b < 4; ++b) {
            h ^= (w >> (8 * b)) & 0xffu;
            h *= 0x100000001b3ull;
        }
    };
    for (const auto& r : rr.itemRuns) { mix(r.x); mix(r.y); }
    for (const auto& r : rr.runs) { mix(r.x); mix(r.y); }
    std::printf("%d %zu %016llx\n", rr.fits ? 1 : 0, rr.runs.size(), static_cast<unsigned long long>(h));
    return 0;
}
