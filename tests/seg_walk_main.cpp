// Stand-alone driver of the segment walker of the attention backward's kernels (csrc/seg_walk.hpp;
// k_spmm and k_attention keep hand-written copies of the loop, which this does not run), built by
// tests/test_seg_walk_cpu.py with the host compiler under -fsanitize=address,undefined. seg_walk is
// instantiated on the host with recording functors and run for the 64 lanes of a wave one after the
// other, for U in {1, 2, 4}, L in {4, 8, 16, 32, 64} and the segment lengths at which the loop
// changes path. A lane's batch record is the entry number it holds (b0 + lane), so the entry a
// shuffle would deliver is known without one. Per (U, L, count) the visiting order is held to:
//   - every entry of [0, count) is used as valid exactly once;
//   - group g's valid entries are g, g + G, ... of each batch, in ascending order;
//   - within a step the U fetches precede the U uses, which come in the same order; a step is one
//     entry wide only where a whole step of U no longer fits;
//   - load(b0) is called once per batch of 64, the next batch's before the current batch's first
//     fetch;
//   - invalid calls occur only in the last step of a batch and only with idx >= nb, and fetch and use
//     agree on `valid`;
//   - fetch is handed the current batch's record and use the entry's slot b0 + idx;
//   - all 64 lanes make the same number of calls (an idle lane still takes part).
// Run with an unroll depth as its argument (or none, for all three); prints "ok <cases>" and exits
// 0, or the first violation and exits 1. (Plain arrays, no containers:
// the test compiles this file every time.)
#include <cstddef>
#include <cstdio>
#include <cstdlib>

#include "seg_walk.hpp"

using bsmr::u32;

namespace {

constexpr u32 MAX_COUNT = 257, MAX_BATCHES = (MAX_COUNT + 63u) / 64u;

enum Kind { LOAD, FETCH, USE };
struct Event {
    Kind kind;
    u32 b0;   // LOAD: the batch; FETCH / USE: the batch the call belongs to
    u32 idx;  // FETCH / USE: the entry's index in its batch
    bool valid;
};
// a lane's calls in order: at most a fetch and a use per entry and per idle tail step, and the loads
// (a run past the end is the sanitizer's to report)
struct Log {
    Event e[2 * (MAX_COUNT + MAX_BATCHES) + MAX_BATCHES];
    size_t n = 0;
    void push(const Event& x) { e[n++] = x; }
};
struct Ent {
    u32 slot;  // b0 + idx of the entry the fetch delivered
    bool valid;
};

int fail(u32 U, u32 L, u32 count, u32 lane, const char* what) {
    printf("U=%u L=%u count=%u lane=%u: %s\n", U, L, count, lane, what);
    return 1;
}

// one lane's walk, the only code instantiated per U; false when a use was handed another entry,
// slot or flag than its fetch delivered
template <u32 U>
bool walk(u32 count, const bsmr::LaneGroups& lg, u32 lane, Log& log) {
    bool ok = true;
    auto load = [&](u32 b0) {
        log.push({LOAD, b0, 0, true});
        return b0 + lane;
    };
    auto fetch = [&](u32 batch, u32 idx, bool valid, Ent& e) {
        const u32 b0 = batch - lane;
        log.push({FETCH, b0, idx, valid});
        e.slot = b0 + idx;
        e.valid = valid;
    };
    auto use = [&](const Ent& e, u32 slot, bool valid) {
        if (e.slot != slot || e.valid != valid) ok = false;
        log.push({USE, slot - slot % 64u, slot % 64u, valid});
    };
    bsmr::seg_walk<U, Ent>(count, lg.G, lg.g, load(0), load, fetch, use);
    return ok;
}

int run_case(u32 U, u32 L, u32 count) {
    const u32 G = 64u / L, batches = (count + 63u) / 64u;
    u32 used[MAX_COUNT] = {};
    size_t calls0 = 0;
    for (u32 lane = 0; lane < 64u; ++lane) {
        const bsmr::LaneGroups lg(L, lane);
        if (lg.L != L || lg.G != G || lg.g != lane / L || lg.l != lane % L) return fail(U, L, count, lane, "geometry");
        Log log;
        const bool ok = U == 1 ? walk<1>(count, lg, lane, log) : U == 2 ? walk<2>(count, lg, lane, log) : walk<4>(count, lg, lane, log);
        if (!ok) return fail(U, L, count, lane, "use was handed another entry than its fetch delivered");
        // the shuffles and butterflies of the functors need all 64 lanes in every call
        if (lane == 0) calls0 = log.n;
        if (log.n != calls0) return fail(U, L, count, lane, "a lane makes fewer calls than lane 0");

        // the loads: batch 0 by the caller, then each later batch once, in order
        size_t loadAt[MAX_BATCHES + 1], loads = 0;
        for (size_t i = 0; i < log.n; ++i)
            if (log.e[i].kind == LOAD) {
                if (loads > MAX_BATCHES || log.e[i].b0 != 64u * loads) return fail(U, L, count, lane, "loads out of order or repeated");
                loadAt[loads++] = i;
            }
        if (loads != (batches ? batches : 1u)) return fail(U, L, count, lane, "not one load per batch of 64");

        // the steps: f fetches (U of a whole step, or one), then the same f entries used in order
        u32 valid[MAX_COUNT];
        size_t nvalid = 0;
        bool closed[MAX_BATCHES + 1] = {};
        u32 lastB0 = 0;
        for (size_t i = 0; i < log.n;) {
            if (log.e[i].kind == LOAD) {
                ++i;
                continue;
            }
            size_t f = 0;
            while (i + f < log.n && log.e[i + f].kind == FETCH) ++f;
            if (f != U && f != 1u) return fail(U, L, count, lane, "a step of neither U fetches nor one");
            const u32 b0 = log.e[i].b0;
            if (b0 % 64u != 0 || b0 >= count || b0 < lastB0) return fail(U, L, count, lane, "fetch from a batch out of turn");
            lastB0 = b0;
            const u32 nb = count - b0 < 64u ? count - b0 : 64u;
            if (closed[b0 / 64u]) return fail(U, L, count, lane, "a step after the batch's partly filled last step");
            if (loadAt[b0 / 64u] > i) return fail(U, L, count, lane, "batch fetched before its load");
            if (b0 + 64u < count && loadAt[b0 / 64u + 1u] > i) return fail(U, L, count, lane, "next batch loaded after a fetch");
            if (i + 2 * f > log.n) return fail(U, L, count, lane, "fetches without their uses");
            for (size_t k = 0; k < f; ++k) {
                const Event &a = log.e[i + k], &b = log.e[i + f + k];
                if (b.kind != USE || a.b0 != b0 || b.b0 != b0 || a.idx != b.idx || a.valid != b.valid)
                    return fail(U, L, count, lane, "uses do not follow their fetches in entry order");
                if (a.idx % G != lg.g) return fail(U, L, count, lane, "an entry of another lane group");
                if (a.valid != (a.idx < nb)) return fail(U, L, count, lane, "valid is not idx < nb");
                if (!a.valid && f != 1u) return fail(U, L, count, lane, "an invalid call inside a whole step of U");
                if (f != U && a.idx / G + U <= nb / G) return fail(U, L, count, lane, "a single step where a whole step of U fits");
                if (!a.valid) closed[b0 / 64u] = true;
                if (a.valid) {
                    if (nvalid == MAX_COUNT) return fail(U, L, count, lane, "more valid uses than entries");
                    valid[nvalid++] = b0 + a.idx;
                }
            }
            i += 2 * f;
        }
        // group g's entries: g, g + G, ... of each batch, ascending, all of them
        size_t n = 0;
        for (u32 b0 = 0; b0 < count; b0 += 64u)
            for (u32 idx = lg.g; idx < 64u && b0 + idx < count; idx += G, ++n)
                if (n >= nvalid || valid[n] != b0 + idx) return fail(U, L, count, lane, "group's entries missing or out of order");
        if (n != nvalid) return fail(U, L, count, lane, "an entry used twice");
        if (lg.l == 0)
            for (size_t k = 0; k < nvalid; ++k) ++used[valid[k]];
    }
    for (u32 s = 0; s < count; ++s)
        if (used[s] != 1u) return fail(U, L, count, 0, "an entry not used exactly once across the lane groups");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    // one unroll depth (argv[1] = 1, 2 or 4), or all three
    const u32 only = argc > 1 ? static_cast<u32>(atoi(argv[1])) : 0;
    u32 cases = 0;
    for (u32 U = 1; U <= 4u; U <<= 1) {
        if (only && U != only) continue;
        for (u32 L = 4; L <= 64u; L <<= 1) {
            const u32 G = 64u / L;
            const u32 counts[] = {0, 1, G - 1, G, G + 1, U * G - 1, U * G, 63, 64, 65, 127, 128, 129, 256, 257};
            for (u32 count : counts) {
                if (run_case(U, L, count)) return 1;
                ++cases;
            }
        }
    }
    printf("ok %u\n", cases);
    return 0;
}
