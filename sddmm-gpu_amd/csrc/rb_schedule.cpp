// rb_schedule.cpp — block geometry and item scheduling of the row-block launch layout, on the host
// alone (rb_schedule.hpp). The cost sums are doubles whose rounding decides cuts: built without
// FMA contraction, and every accumulation keeps its order, so every rank of a multi-GPU run and
// every host thread count derive the same layout.
#include "rb_schedule.hpp"

#include <cmath>
#include <cstdio>
#include <queue>
#include <type_traits>
#include <utility>

namespace bsmr {

using u32 = uint32_t;
using u64 = uint64_t;

u32 rowblock_rows(u32 rowBytes, u32 lds_kb, u32 R) {
    // (rows of <= 512 B: the workgroup's last LDS word is the piece-batch counter of k_sddmm_rb /
    // k_sddmm_rb_pair, so a whole-LDS budget leaves it out; an 80 KiB image is caught where the
    // block size is final)
    u64 bytes = static_cast<u64>(lds_kb) * 1024;
    if (rowBytes <= 512 && bytes >= 160u * 1024u) bytes = 160u * 1024u - 16u;
    u32 rb = static_cast<u32>(bytes / rowBytes / 16 * 16);
    rb = std::min<u32>(std::max<u32>(rb, 16), 1024);
    return std::min<u32>(rb, std::max<u32>((R + 15) / 16 * 16, 16));
}

RbGeometry rb_geometry(u32 rowBytes, u32 Rs, u32 n0, u32 NS, u32 nnz, int cus, bool orig, bool cols,
                       const Knobs& k) {
    RbGeometry g;
    g.rowBytes = rowBytes;
    g.orig = orig;
    g.cols = cols;
    // staged output (results through LDS, written per item in CSR order) for large P
    g.stagedWanted = k.out_staged == 1 || (k.out_staged == -1 && 4ull * nnz > k.out_staged_min);
    const bool stagedWanted = g.stagedWanted;
    // staged-output budget by row size (item_sched): 1 KiB rows take an 80 KiB image (two
    // workgroups per CU, results stored directly), 2 KiB rows the whole 160 KiB (mycielskian K =
    // 256 / 512: 379 -> 358 us and 896 -> 771 us against the 120 KiB staged image;
    // profiles/r03f/itemcal); 512-byte rows keep the tuned 120 KiB staged image (C4)
    const u32 stagedKb = !k.item_cost_cuts || rowBytes <= 512 ? k.rb_lds_kb_staged : rowBytes <= 1024 ? 80u : 160u;
    // 2 KiB rows (fp32 K = 512, fp16/bf16 K = 1024) take the whole-LDS image and 8 MiB column
    // ranges whatever P's size: an item's A image is 80 rows x 2 KiB, and fewer, wider ranges
    // restage it less (mycielskian14 / 15 / 16 K = 512: 100 -> 87, 253 -> 238, 735 -> 716 us;
    // 1 KiB rows lose with 8 MiB ranges: mycielskian16 K = 256 358 -> 468 us; profiles/r03u).
    // Sparse rows (< 64 stored entries per row) keep the small-row-block rule below (Trefethen
    // K = 512: 48-row blocks 48.1 us, 80-row blocks 51.5 us; profiles/r03v)
    const bool bigRows = k.item_cost_cuts && rowBytes >= 2048 && n0 >= 64ull * Rs;
    const u32 ldsKb = (stagedWanted || bigRows) && !k.rb_lds_user ? stagedKb : k.rb_lds_kb;
    // staged 512-byte rows (C4 reddit-like x1 fp32 K = 128): 8 MiB ranges too, half the A
    // restaging for a B range twice the L2 (4.01 -> 3.89 ms over three alternating runs,
    // profiles/r03y; C3 fp16 K = 256 neutral)
    // ... but at least two ranges per XCD when its B share exceeds its 4 MiB L2: one range of the
    // whole share ran C4 x0.5 (7.5 MiB per XCD) at 1.33 ms against 1.00 ms with two
    // (profiles/r04x); x1 keeps two 7.5 MiB ranges; a share that fits the L2 stays one range
    // (mycielskian16 K = 128, 3 MiB per XCD: 166 us against 181 us with two; profiles/r04zr)
    const bool staged512 = stagedWanted && k.item_cost_cuts && rowBytes == 512;
    const double shareKb = static_cast<double>(NS) * rowBytes / RB_XCDS / 1024.0;
    g.l2Kb = k.l2_range_user ? k.l2_range_kb
             : staged512 ? (shareKb > 4096.0 ? std::min<u32>(8192u, static_cast<u32>(std::ceil(shareKb / 2)) + 1)
                                             : 8192u)
             : bigRows ? 8192u
             : stagedWanted ? k.l2_range_kb_staged : k.l2_range_kb;
    u32 RBr = rowblock_rows(rowBytes, ldsKb, Rs);
    {
        // sparse rows (< 64 stored entries per row: banded / FEM patterns) keep their row blocks
        // whole, one item each; when there are more row blocks than workgroup slots, use the
        // smallest row block that needs no more rounds of slots, so the last round is full
        // (cop20k-like C3: 421 blocks of 288 rows = 1.6 rounds -> 505 blocks of 240 rows)
        const size_t lds0 = static_cast<size_t>(RBr) * rowBytes;
        const u32 slots = static_cast<u32>(cus) * (lds0 > 80 * 1024 ? 1u : 2u);
        const u32 nRB0 = (Rs + RBr - 1) / std::max<u32>(RBr, 1);
        // (column blocks keep the whole image: their point is long row runs per block)
        if (cols) {
        } else if (Rs && n0 < 64ull * Rs && nRB0 > slots) {
            const u32 rounds = (nRB0 + slots - 1) / slots;
            const u32 rb = (Rs + rounds * slots - 1) / (rounds * slots);
            RBr = std::min(RBr, std::max<u32>(16, (rb + 15) / 16 * 16));
        } else if (Rs && n0 < 64ull * Rs && k.small_sparse_rb) {
            // fewer row blocks than slots: a block would be cut into chunks that each restage
            // its whole image for a few entries (Trefethen_20000 K = 64: 35 blocks of 576 rows in
            // 257 items, 15.2 us). One block per slot instead, at two workgroups per CU when the
            // image fits 80 KiB (48-row blocks in 512 items: 8.9 us; profiles/r03e/itemcal)
            const u32 s2 = static_cast<u32>(cus) * 2u;
            const u32 rb2 = std::max<u32>(16, ((Rs + s2 - 1) / s2 + 15) / 16 * 16);
            const u32 rb1 = std::max<u32>(16, ((Rs + cus - 1) / cus + 15) / 16 * 16);
            if (static_cast<size_t>(rb2) * rowBytes <= 80 * 1024) RBr = std::min(RBr, rb2);
            else RBr = std::min(RBr, rb1);
        }
    }
    if (Rs && (cols || n0 >= 64ull * Rs) && !(k.diag & 32768)) {
        // non-sparse rows: the same number of row blocks, of equal size (a multiple of 16), so
        // no short last block and every item stages the smallest image that count allows (C2
        // nips-like: 5 x 288 + 60 rows -> 5 x 256 + 220, 10.80 -> 10.63 us; BSMR_DIAG & 32768
        // keeps the LDS-budget size)
        const u32 nb0 = (Rs + RBr - 1) / RBr;
        RBr = std::min(RBr, std::max<u32>(16, ((Rs + nb0 - 1) / nb0 + 15) / 16 * 16));
    }
    // column blocks: the largest image the workgroup's LDS takes (fewer blocks, longer row runs:
    // C2 nips-like 288 -> 304 columns, 78.7 K -> 75.8 K pieces)
    // (staged output keeps its budget: the result slots live past the image)
    if (cols && !k.rb_lds_user && !stagedWanted && Rs) {
        // (batches never: no piece-batch counter to keep free, so the image may fill the LDS)
        const u32 rfull = std::min<u32>(std::min<u32>(160u * 1024u / rowBytes / 16 * 16, 1024),
                                        std::max<u32>((Rs + 15) / 16 * 16, 16));
        const u32 rmax = k.batches == 0 ? rfull : rowblock_rows(rowBytes, 160, Rs), nb0 = (Rs + rmax - 1) / rmax;
        RBr = std::min(rmax, std::max<u32>(16, ((Rs + nb0 - 1) / nb0 + 15) / 16 * 16));
    }
    if (k.rb_rows_force > 0)  // tuning: rows per block (a multiple of 16 within the LDS budget)
        RBr = std::min(rowblock_rows(rowBytes, 160, Rs),
                       std::max<u32>(16, (static_cast<u32>(k.rb_rows_force) + 15) / 16 * 16));
    // rows of <= 512 B: an image of exactly 80 KiB would fill a 512-thread workgroup's LDS, whose
    // last word is the piece-batch counter (160 KiB images are excluded by rowblock_rows)
    if (rowBytes <= 512 && static_cast<size_t>(RBr) * rowBytes == 80u * 1024u && RBr > 16) RBr -= 16;
    g.RB = RBr;
    g.nRB = std::max<u32>(1, (Rs + RBr - 1) / RBr);
    g.lds = static_cast<size_t>(RBr) * rowBytes;
    g.NT = g.lds > 80 * 1024 ? 1024 : 512;
    // k_sddmm_rb takes 160 KiB (1024 threads) or 80 KiB (512) of LDS per workgroup
    const u32 wgPerCU = g.NT == 1024 ? 1 : 2;
    g.perBucket = std::max<u32>(1, static_cast<u32>(cus) * wgPerCU / RB_XCDS);
    // column ranges: NCR = 8 m ranges of (nearly) equal residual count; XCD x owns ranges
    // [x m, (x + 1) m). m makes one range's B columns (N rowBytes / NCR) fit an L2 budget: the
    // items of an XCD are ordered by range, so the B columns an item gathers were brought into
    // that XCD's L2 by the items before it (graph matrices: B is gathered once per row block and
    // column run, from L2 instead of the Infinity Cache)
    g.m = std::max<u32>(1, static_cast<u32>(std::ceil(
        static_cast<double>(NS) * rowBytes / RB_XCDS / (static_cast<double>(g.l2Kb) * 1024.0))));
    // staged output: the LDS past the A image (the launch takes 160 / 80 KiB) holds an item's
    // results when it has room for >= 1024 of them; larger items are cut to fit
    const size_t ldsDyn = (g.NT == 1024 ? 160u : 80u) * 1024u;
    // (the last 16 bytes: the piece-batch counter)
    g.outCap = ldsDyn > g.lds + 16 ? static_cast<u32>((ldsDyn - g.lds - 16) / 4) : 0u;
    g.staged = stagedWanted && g.outCap >= 1024;
    return g;
}

namespace {

constexpr u32 CM = RB_COL_MASK;

// The column-run pieces of entries [e0, e1): cut at column changes and every piece_max entries;
// f(first entry, length, column) per piece, in order; an f that returns bool ends the walk with
// false.
template <class F>
void for_each_piece(const u32* ent, u32 e0, u32 e1, u32 piece_max, F&& f) {
    for (u32 e = e0; e < e1;) {
        const u32 col = ent[e] & CM;
        u32 g = e + 1;
        while (g < e1 && g - e < piece_max && (ent[g] & CM) == col) ++g;
        if constexpr (std::is_void_v<decltype(f(e, g - e, col))>)
            f(e, g - e, col);
        else if (!f(e, g - e, col))
            return;
        e = g;
    }
}

// One XCD's workgroup slots: an item starts when a slot frees, in the order pushed.
class SlotModel {
public:
    explicit SlotModel(u32 slots) {
        for (u32 k = 0; k < slots; ++k) free_.push(0.0);
    }
    double earliest() const { return free_.top(); }  // when the next item would start
    void push(double cost) {
        const double t = free_.top() + cost;
        free_.pop();
        free_.push(t);
        end_ = std::max(end_, t);
    }
    double makespan() const { return end_; }

private:
    std::priority_queue<double, std::vector<double>, std::greater<double>> free_;
    double end_ = 0.0;
};

// split q chunks over segments by cost (largest remainder); every non-empty segment gets >= 1,
// and >= ceil(cost / cap) when cap > 0 (no chunk above cap; the total may then exceed q)
std::vector<u32> apportion(const std::vector<double>& cost, u32 q, double cap = 0.0) {
    const size_t n = cost.size();
    std::vector<u32> out(n, 0);
    double tot = 0;
    for (double c : cost) tot += c;
    if (tot <= 0) return out;
    std::vector<std::pair<double, size_t>> frac;
    u32 used = 0;
    for (size_t i = 0; i < n; ++i) {
        if (cost[i] <= 0) continue;
        const double ideal = q * cost[i] / tot;
        out[i] = std::max<u32>(1, static_cast<u32>(std::floor(ideal)));
        if (cap > 0) out[i] = std::max<u32>(out[i], static_cast<u32>(std::ceil(cost[i] / cap)));
        used += out[i];
        // capped: rank by what is still missing; uncapped: by the fractional part (the round-2
        // rule, so BSMR_ITEM_SCHED=0 BSMR_ITEM_CAP=0 reproduces the round-2 item lists)
        frac.push_back({cap > 0 ? ideal - out[i] : ideal - std::floor(ideal), i});
    }
    std::stable_sort(frac.begin(), frac.end(),
                     [](const auto& a, const auto& b) { return a.first > b.first; });
    for (size_t k = 0; used < q && k < frac.size(); ++k, ++used) ++out[frac[k].second];
    return out;
}

// Static piece order of one row-block item (piece_balance). The kernel deals phase ph's
// pieces [ph NG, (ph + 1) NG) to row-groups gr, reversed in odd phases (rb_kernel.hpp: piece
// ph NG + (ph odd ? NG - 1 - gr : gr)); a wave's 64 / G row-groups run a phase in lockstep, so a
// wave pays per phase its longest piece plus one gather (w entry-steps, the item cost model's
// piece weight). With the pieces longest first in position order, the waves that also run the
// short last phase end last. Here the same pieces, sorted longest first, go out in runs — one
// run per (wave, phase) bucket, as many pieces as that bucket has positions — always to the wave
// whose running cost is lowest (LPT over the buckets), so waves with two phases get shorter runs.
void balance_pieces(std::vector<RbPiece>& pcs, u32 NT, u32 G, double w) {
    const u32 NG = NT / G, GW = 64 / G, NW = NT / 64;
    const u32 np = static_cast<u32>(pcs.size());
    if (np <= NG) return;  // one phase: every wave has one bucket already in cost order
    const u32 nph = (np + NG - 1) / NG;
    struct Bucket {
        u32 ph, cap;
        std::vector<u32> pos;  // the positions (piece indices) of its row-groups
    };
    std::vector<std::vector<Bucket>> wb(NW);
    for (u32 ph = 0; ph < nph; ++ph)
        for (u32 wv = 0; wv < NW; ++wv) {
            Bucket bk{ph, 0, {}};
            for (u32 gr = wv * GW; gr < (wv + 1) * GW; ++gr) {
                const u32 pos = ph * NG + ((ph & 1) ? NG - 1 - gr : gr);
                if (pos < np) bk.pos.push_back(pos);
            }
            bk.cap = static_cast<u32>(bk.pos.size());
            if (bk.cap) wb[wv].push_back(std::move(bk));
        }
    // buckets of a wave largest first
    for (auto& v : wb)
        std::stable_sort(v.begin(), v.end(), [](const Bucket& a, const Bucket& b) { return a.cap > b.cap; });
    std::vector<double> cost(NW, 0.0);
    std::vector<u32> next(NW, 0);
    std::vector<RbPiece> out(np);
    u32 k = 0;  // pcs sorted longest first
    while (k < np) {
        u32 best = NW;
        for (u32 wv = 0; wv < NW; ++wv)
            if (next[wv] < wb[wv].size() && (best == NW || cost[wv] < cost[best])) best = wv;
        const Bucket& bk = wb[best][next[best]++];
        cost[best] += static_cast<double>((pcs[k].y >> 22) + 1) + w;
        for (u32 pos : bk.pos) out[pos] = pcs[k++];
    }
    pcs.swap(out);
}

// Column cuts: cuts[x] = first column of range x (NCR + 1 values, cuts[NCR] = NS), the ranges
// carrying equal weight.
// column weight: its entries, plus (item_sched) piece_weight per column-run piece it heads, so the
// XCDs' ranges carry equal modeled cost rather than equal entry counts (mycielskian: the last
// XCD's range carried 10 % more piece work and ended 10 % later).
// Integer counts per column — entries, and column-run pieces per row block — then cnt = entries +
// piece_weight x pieces: exact whatever the host's thread count. Each host thread takes a stripe
// of columns and finds its part of every row block's column-sorted entries by binary search:
// N + 1 counters in all, not one vector per row-block chunk.
std::vector<u32> column_cuts(const RbScheduleIn& in, u32 NCR) {
    const u32 NS = in.NS, nRB = in.geom.nRB, piece_max = in.knobs->piece_max;
    const u32* ent = in.entries;
    const u32* rbEnd = in.rbEnd;
    std::vector<u32> cuts(NCR + 1, NS);
    cuts[0] = 0;
    std::vector<u32> ecount(NS + 1, 0), scount(NS + 1, 0);
    const u32 NSTR = 64;
    par_for(NSTR, [&](unsigned, size_t s0, size_t s1) {
        for (size_t st = s0; st < s1; ++st) {
            const u32 c0 = static_cast<u32>(static_cast<u64>(NS) * st / NSTR);
            const u32 c1 = static_cast<u32>(static_cast<u64>(NS) * (st + 1) / NSTR);
            if (c0 == c1) continue;
            for (u32 b = 0; b < nRB; ++b) {
                const u32* lo = ent + (b ? rbEnd[b - 1] : 0u);
                const u32* hi = ent + rbEnd[b];
                const auto byCol = [](u32 m, u32 c) { return (m & CM) < c; };
                const u32* p = std::lower_bound(lo, hi, c0, byCol);
                const u32* q = std::lower_bound(p, hi, c1, byCol);
                for_each_piece(ent, static_cast<u32>(p - ent), static_cast<u32>(q - ent), piece_max,
                               [&](u32, u32 len, u32 c) {
                                   ecount[c] += len;
                                   ++scount[c];
                               });
            }
        }
    }, 1, in.threads);
    std::vector<double> cnt(NS + 1, 0.0);
    for (u32 c = 0; c < NS; ++c)
        cnt[c] = static_cast<double>(ecount[c]) +
                 (in.knobs->item_cost_cuts ? in.knobs->piece_weight * scount[c] : 0.0);
    double tot = 0;
    for (u32 c = 0; c < NS; ++c) tot += cnt[c];
    double run = 0;
    u32 x = 1;
    for (u32 c = 0; c < NS && x < NCR; ++c) {
        while (x < NCR && run >= tot * x / NCR) cuts[x++] = c;
        run += cnt[c];
    }
    for (; x < NCR; ++x) cuts[x] = NS;
    return cuts;
}

// segments (rb, range k), index rb * NCR + k: entries [e0, e1) of rb in range k, 1/NCR of rb's
// kept tiles [t0, t1), pc column-run pieces; cost = entries + piece_weight per piece (one B
// column each) + 16 per tile
struct Segments {
    u32 NCR = 0;
    std::vector<u32> e0, e1, t0, t1, pc;
    std::vector<double> cost;
    std::vector<u64> piecesRB;  // pieces per row block
};

Segments build_segments(const RbScheduleIn& in, const std::vector<u32>& cuts, u32 NCR) {
    const u32 nRB = in.geom.nRB, piece_max = in.knobs->piece_max;
    const double piece_weight = in.knobs->piece_weight;
    const u32* ent = in.entries;
    const size_t nseg = static_cast<size_t>(nRB) * NCR;
    Segments s;
    s.NCR = NCR;
    s.e0.resize(nseg);
    s.e1.resize(nseg);
    s.t0.resize(nseg);
    s.t1.resize(nseg);
    s.pc.assign(nseg, 0);
    s.cost.resize(nseg);
    s.piecesRB.assign(nRB, 0);
    par_for(nRB, [&](unsigned, size_t bb0, size_t bb1) {
        for (u32 b = static_cast<u32>(bb0); b < bb1; ++b) {
            const u32 eb0 = b ? in.rbEnd[b - 1] : 0, eb1 = in.rbEnd[b];
            const u32 t0 = in.keptBegin ? in.keptBegin[b] : 0;
            const u32 nt = in.keptBegin ? in.keptBegin[b + 1] - t0 : 0;
            u32 lo = eb0;
            for (u32 k = 0; k < NCR; ++k) {
                const size_t i = static_cast<size_t>(b) * NCR + k;
                const u32 hi = k + 1 < NCR
                                   ? static_cast<u32>(std::lower_bound(ent + lo, ent + eb1, cuts[k + 1],
                                                                       [](u32 v, u32 c) { return (v & CM) < c; }) -
                                                      ent)
                                   : eb1;
                s.e0[i] = lo;
                s.e1[i] = hi;
                for_each_piece(ent, lo, hi, piece_max, [&](u32, u32, u32) { ++s.pc[i]; });
                s.piecesRB[b] += s.pc[i];
                lo = hi;
                s.t0[i] = t0 + static_cast<u32>(static_cast<u64>(nt) * k / NCR);
                s.t1[i] = t0 + static_cast<u32>(static_cast<u64>(nt) * (k + 1) / NCR);
                s.cost[i] = (s.e1[i] - s.e0[i]) + piece_weight * s.pc[i] + 16.0 * (s.t1[i] - s.t0[i]);
            }
        }
    }, 16, in.threads);
    return s;
}

// the XCDs' item lists: items {rb, ta, tb, ea}, their entry ends, and each item's modeled cost
// (its entries + pieces + 16 per kept tile + staging (piece_weight per row) + item_fixed)
struct Lists {
    std::vector<std::vector<RbItem>> items;
    std::vector<std::vector<u32>> ends;
    std::vector<std::vector<double>> cost;
    void assign(size_t n) {
        items.assign(n, {});
        ends.assign(n, {});
        cost.assign(n, {});
    }
    void resize(size_t n) {
        items.resize(n);
        ends.resize(n);
        cost.resize(n);
    }
    void push(u32 x, const RbItem& it, u32 end, double c) {
        items[x].push_back(it);
        ends[x].push_back(end);
        cost[x].push_back(c);
    }
};

// Chunk planning. A row block is split by the column ranges (its items then read B from their own
// XCD's L2) when it is big enough for >= 8 items of a one-round launch, or (m > 1) when its
// column runs would gather more B rows than NCR restagings of its A rows cost; a smaller one
// (e.g. banded matrices: many row blocks of few entries) is cut along its whole column-sorted
// entry list, and its items balance the XCD list lengths. Item counts come from
// largest-remainder apportionment; Q is one round of workgroup slots (fewer if items would
// drop below ~128 cost units), or whole rounds when the split segments need more items.
class ChunkPlanner {
public:
    ChunkPlanner(const RbScheduleIn& in, const Segments& seg);
    // the lists under the cost cap the slot model runs fastest (or the fixed item_cap)
    Lists plan();

private:
    void cuts_by_cost(u32 e0, u32 ne, u32 nch, double tot);
    void emit(u32 xl, u32 b, u32 e0, u32 ne, u32 t0, u32 nt, u32 nch, double rcost);
    void place_unsplit(size_t nsp);
    double build_lists(double capv);

    const RbScheduleIn& in_;
    const RbGeometry& g_;
    const Knobs& k_;
    const Segments& seg_;
    const u32 nRB_, NCR_;
    double total_ = 0, target_ = 0, cap_ = 0, splitTotal_ = 0;
    u32 Q1_ = 0, Q_ = 0, segMax_ = 0, qEach_ = 0, qSplit_ = 0;
    std::vector<double> cb_, cu_;  // per row block: its cost; the same when unsplit, else 0
    std::vector<char> split_;
    std::vector<u32> nu_;  // per unsplit row block: its chunks
    // scratch of cuts_by_cost: a range's chunk boundaries and the chunks' costs (entries + pieces)
    std::vector<u32> ecut_, ecut2_;
    std::vector<double> ccost_, ccost2_;
    Lists lists_;
};

ChunkPlanner::ChunkPlanner(const RbScheduleIn& in, const Segments& seg)
    : in_(in), g_(in.geom), k_(*in.knobs), seg_(seg), nRB_(in.geom.nRB), NCR_(seg.NCR) {
    const u32 m = g_.m;
    for (double c : seg_.cost) total_ += c;
    Q1_ = g_.perBucket * RB_XCDS;
    Q_ = std::max<u32>(1, std::min<u32>(Q1_, static_cast<u32>(total_ / 128.0)));
    target_ = total_ / Q_;
    // no chunk above item_cap x one slot's share of a round (0: off): a row block of one hub row
    // (mycielskian: 8 K single-entry pieces in one item against a 6 K-entry median) otherwise
    // outlasts the whole launch (profiles/r03e/itemcal). 1x would force extra items into a
    // second round wherever a segment sits just above the mean (C2: 11 -> 17 us)
    cap_ = (k_.item_cap < 0 ? 2.0 : k_.item_cap) * total_ / Q1_;
    cb_.assign(nRB_, 0.0);
    split_.assign(nRB_, 0);
    std::vector<u32> segX(RB_XCDS, 0);  // non-empty split segments per XCD
    // column blocks whose whole gathered operand (A) fits half an XCD's L2 (C2: 768 KiB): no
    // block is split by range, so each block's items run on one XCD (contiguous eighths) and its
    // B image comes into that L2 once — split by range, every XCD would pull every block's image
    // from the Infinity Cache (8 x B per launch) to save gathers of an A that is L2-resident anyway
    const bool colsLocal = g_.cols && static_cast<u64>(in_.NS) * g_.rowBytes <= (2ull << 20) && !(k_.diag & 4096);
    for (u32 b = 0; b < nRB_; ++b) {
        for (u32 k = 0; k < NCR_; ++k) cb_[b] += seg_.cost[static_cast<size_t>(b) * NCR_ + k];
        split_[b] = !colsLocal && (cb_[b] >= RB_XCDS * target_ ||
                                   (m > 1 && seg_.piecesRB[b] >= static_cast<u64>(NCR_) * g_.RB));
        if (!split_[b]) continue;
        splitTotal_ += cb_[b];
        for (u32 k = 0; k < NCR_; ++k)
            segX[k / m] += seg_.cost[static_cast<size_t>(b) * NCR_ + k] > 0;
    }
    // the same quota for every XCD (the column cuts balance them): an extra item in one list
    // would start another round of slots on that XCD
    segMax_ = *std::max_element(segX.begin(), segX.end());
    if (segMax_ * RB_XCDS > Q_) Q_ = (segMax_ * RB_XCDS + Q1_ - 1) / Q1_ * Q1_;
    qEach_ = std::max<u32>(segMax_, static_cast<u32>(std::llround(
        static_cast<double>(Q_ / RB_XCDS) * (total_ > 0 ? splitTotal_ / total_ : 0.0))));
    qSplit_ = qEach_ * RB_XCDS;
    cu_.assign(nRB_, 0.0);
    for (u32 b = 0; b < nRB_; ++b) cu_[b] = split_[b] ? 0.0 : cb_[b];
}

// chunk k of an entry range: cut where the running cost (1 per entry + piece_weight per
// column-run piece start) crosses k / nch of the range's cost, so chunks of single-entry
// pieces get fewer entries than chunks of long runs; a chunk above the staged-output
// capacity is then cut entry-evenly into as many as it needs (an entry-even cut of the whole
// range would put a hub row's single-entry run into one chunk of 5x the others' cost).
// tot = the range's entries + piece_weight per piece (known from its segments' costs), so
// one pass finds the cuts; ccost_ = the chunks' costs (entries + pieces) for the slot model
void ChunkPlanner::cuts_by_cost(u32 e0, u32 ne, u32 nch, double tot) {
    const double piece_weight = k_.piece_weight;
    ecut_.assign(nch + 1, e0 + ne);
    ecut_[0] = e0;
    ccost_.assign(nch, nch ? tot / nch : 0.0);
    if (nch > 1 && !k_.item_cost_cuts) {
        for (u32 k = 1; k < nch; ++k) ecut_[k] = e0 + static_cast<u32>(static_cast<u64>(ne) * k / nch);
    } else if (nch > 1) {
        double acc = 0, last = 0;
        u32 k = 1;
        for_each_piece(in_.entries, e0, e0 + ne, k_.piece_max, [&](u32 first, u32 len, u32) {
            for (u32 e = first; e < first + len && k < nch; ++e) {
                while (k < nch && acc >= tot * k / nch) {
                    ecut_[k] = e;
                    ccost_[k - 1] = acc - last;
                    last = acc;
                    ++k;
                }
                acc += 1.0 + (e == first ? piece_weight : 0.0);
            }
            return k < nch;  // the last cut is found: the rest of the range is the last chunk
        });
        // the chunk from the last cut runs to the range's end; cuts never reached (k < nch)
        // leave empty chunks behind it
        for (u32 j = k; j < nch; ++j) ccost_[j] = 0.0;
        ccost_[k - 1] = std::max(0.0, tot - last);
    }
    if (!g_.staged) return;
    const u32 outCap = g_.outCap;
    ecut2_.assign(1, e0);
    ccost2_.clear();
    for (u32 j = 0; j < nch; ++j) {
        const u32 a = ecut_[j], len = ecut_[j + 1] - a, parts = std::max<u32>(1, (len + outCap - 1) / outCap);
        for (u32 q = 1; q <= parts; ++q) {
            ecut2_.push_back(a + static_cast<u32>(static_cast<u64>(len) * q / parts));
            ccost2_.push_back(ccost_[j] / parts);
        }
    }
    ecut_.swap(ecut2_);
    ccost_.swap(ccost2_);
}

// the items of row block b's entries [e0, e0 + ne) and kept tiles [t0, t0 + nt), in nch chunks
// (more when staged output needs it), appended to list xl; rcost = the range's entries + pieces
void ChunkPlanner::emit(u32 xl, u32 b, u32 e0, u32 ne, u32 t0, u32 nt, u32 nch, double rcost) {
    if (g_.staged) nch = std::max<u32>(nch, (ne + g_.outCap - 1) / g_.outCap);
    cuts_by_cost(e0, ne, nch, rcost);
    nch = static_cast<u32>(ecut_.size() - 1);
    for (u32 k = 0; k < nch; ++k) {
        const u32 ea = ecut_[k];
        const u32 eb = ecut_[k + 1];
        const u32 ta = t0 + static_cast<u32>(static_cast<u64>(nt) * k / nch);
        const u32 tb = t0 + static_cast<u32>(static_cast<u64>(nt) * (k + 1) / nch);
        if (ea == eb && ta == tb) continue;
        lists_.push(xl, RbItem{b, ta, tb, ea}, eb,
                    ccost_[k] + 16.0 * (tb - ta) + k_.piece_weight * g_.RB + k_.item_fixed);
    }
}

// unsplit row blocks: their nsp items, in row-block order in the staging list (index RB_XCDS), go
// to the list with the fewest items, so no XCD runs an extra round (a contiguous range of blocks
// per XCD, for L2 sharing of banded columns, measured 7 % slower on the cop20k-like C3 pattern)
void ChunkPlanner::place_unsplit(size_t nsp) {
    const u32 spare = RB_XCDS;
    const bool contig = (g_.orig || g_.cols) && k_.orig_contig && qSplit_ == 0;
    if (k_.item_lpt && !contig && nsp) {
        // list scheduling: each XCD runs its list on perBucket slots, an item starting when a
        // slot frees (in list order). The XCD lists' split items are simulated first; then
        // the unsplit items, heaviest first, each go to the XCD where it starts earliest
        // (ties: fewer items, lower index), appended to that list, which keeps every list in
        // descending order of its unsplit items' cost
        std::vector<SlotModel> free(RB_XCDS, SlotModel(g_.perBucket));
        for (u32 x = 0; x < RB_XCDS; ++x)
            for (double c : lists_.cost[x]) free[x].push(c);
        std::vector<std::pair<double, size_t>> ord(nsp);
        for (size_t i = 0; i < nsp; ++i) ord[i] = {lists_.cost[spare][i], i};
        std::stable_sort(ord.begin(), ord.end(),
                         [](const auto& a, const auto& b) { return a.first > b.first; });
        for (const auto& [c, i] : ord) {
            u32 x = 0;
            for (u32 y = 1; y < RB_XCDS; ++y) {
                const double ty = free[y].earliest(), tx = free[x].earliest();
                if (ty < tx || (ty == tx && lists_.items[y].size() < lists_.items[x].size())) x = y;
            }
            free[x].push(c);
            lists_.push(x, lists_.items[spare][i], lists_.ends[spare][i], c);
        }
    } else {
        for (size_t next = 0; next < nsp; ++next) {
            u32 x = 0;  // the list with the fewest items (ties: lowest index)
            for (u32 y = 1; y < RB_XCDS; ++y)
                if (lists_.items[y].size() < lists_.items[x].size()) x = y;
            // original-order blocks (orig_contig): XCD x takes the x-th contiguous eighth, so
            // the band's B rows of neighbouring blocks stay in one L2
            if (contig) x = static_cast<u32>(next * RB_XCDS / nsp);
            lists_.push(x, lists_.items[spare][next], lists_.ends[spare][next], lists_.cost[spare][next]);
        }
    }
}

// the XCD lists for one cost cap (0: none); returns the modeled makespan: each XCD runs its
// list on perBucket slots, an item starting when a slot frees (in list order)
double ChunkPlanner::build_lists(const double capv) {
    const u32 m = g_.m;
    const double piece_weight = k_.piece_weight;
    lists_.assign(RB_XCDS);
    nu_ = apportion(cu_, Q_ > qSplit_ ? Q_ - qSplit_ : 0u, capv);
    for (u32 x = 0; x < RB_XCDS; ++x) {
        // XCD x's segments in (range, row block) order
        std::vector<double> c(static_cast<size_t>(m) * nRB_, 0.0);
        for (u32 j = 0; j < m; ++j)
            for (u32 b = 0; b < nRB_; ++b)
                c[static_cast<size_t>(j) * nRB_ + b] =
                    split_[b] ? seg_.cost[static_cast<size_t>(b) * NCR_ + x * m + j] : 0.0;
        const std::vector<u32> nch = apportion(c, qEach_, capv);
        for (u32 j = 0; j < m; ++j)
            for (u32 b = 0; b < nRB_; ++b) {
                const size_t i = static_cast<size_t>(b) * NCR_ + x * m + j;
                const u32 q = nch[static_cast<size_t>(j) * nRB_ + b];
                if (q)
                    emit(x, b, seg_.e0[i], seg_.e1[i] - seg_.e0[i], seg_.t0[i], seg_.t1[i] - seg_.t0[i], q,
                         (seg_.e1[i] - seg_.e0[i]) + piece_weight * seg_.pc[i]);
            }
    }
    const u32 spare = RB_XCDS;  // staging list index
    lists_.resize(RB_XCDS + 1);
    for (u32 b = 0; b < nRB_; ++b) {
        if (!nu_[b]) continue;
        const size_t i0 = static_cast<size_t>(b) * NCR_, i1 = i0 + NCR_ - 1;
        double rc = 0.0;
        for (size_t i = i0; i <= i1; ++i) rc += (seg_.e1[i] - seg_.e0[i]) + piece_weight * seg_.pc[i];
        emit(spare, b, seg_.e0[i0], seg_.e1[i1] - seg_.e0[i0], seg_.t0[i0], seg_.t1[i1] - seg_.t0[i0], nu_[b], rc);
    }
    place_unsplit(lists_.items[spare].size());
    lists_.resize(RB_XCDS);
    double ms = 0.0;
    for (u32 x = 0; x < RB_XCDS; ++x) {
        SlotModel slots(g_.perBucket);
        for (double c : lists_.cost[x]) slots.push(c);
        ms = std::max(ms, slots.makespan());
    }
    return ms;
}

Lists ChunkPlanner::plan() {
    // the cap: item_cap x one slot's share, or (auto, item_sched, up to 32 M entries) the
    // multiple in {2, 1.5, 1.25, 1} whose lists the slot model runs fastest (a one-round launch
    // ends with its longest item: mycielskian15 K = 256, 2x cap 144 us; C2's segments sit just
    // above the mean, where 1x would open a second round)
    double capUse = cap_;
    if (k_.item_lpt && k_.item_cap < 0 && in_.n <= (1u << 25)) {
        double best = -1.0;
        for (const double f : {2.0, 1.5, 1.25, 1.0}) {
            const double msf = build_lists(f * total_ / Q1_);
            if (best < 0 || msf < 0.995 * best) {
                best = msf;
                capUse = f * total_ / Q1_;
            }
        }
    }
    const double msUse = build_lists(capUse);
    if (k_.diag & 1024) {  // layout debug (host stderr)
        std::fprintf(stderr, "[rb layout] RB %u NT %u nRB %u m %u Q1 %u Q %u total %.0f target %.0f cap %.0f (used %.0f, model makespan %.0f) "
                     "splitTotal %.0f qEach %u segMax %u\n", g_.RB, g_.NT, nRB_, g_.m, Q1_, Q_, total_, target_, cap_, capUse, msUse,
                     splitTotal_, qEach_, segMax_);
        for (u32 b = 0; b < nRB_; ++b)
            if (cb_[b] > 2 * target_)
                std::fprintf(stderr, "[rb layout]   block %u cost %.0f split %d nu %u\n", b, cb_[b], split_[b], nu_[b]);
    }
    return std::move(lists_);
}

// launch order: list position j of XCD x at j * 8 + x, the lists padded to one length with zero
// items (staged layouts: an even number of positions, so the launch can pair them; k_sddmm_rb)
void interleave(const Lists& lists, bool staged, std::vector<RbItem>& items, std::vector<u32>& ends) {
    size_t nmax = 0;
    for (const auto& l : lists.items) nmax = std::max(nmax, l.size());
    if (staged) nmax = (nmax + 1) & ~static_cast<size_t>(1);
    items.assign(nmax * RB_XCDS, RbItem{0, 0, 0, 0});
    ends.assign(nmax * RB_XCDS, 0);
    for (u32 x = 0; x < RB_XCDS; ++x)
        for (size_t j = 0; j < lists.items[x].size(); ++j) {
            items[j * RB_XCDS + x] = lists.items[x][j];
            ends[j * RB_XCDS + x] = lists.ends[x][j];
        }
}

// column-run pieces: each item's entries [e0, e1) cut at column changes and every
// piece_max (<= RB_PIECE_MAX) entries; piece {first entry, column | (length - 1) << 22}. A workgroup's NG
// row-groups take one piece each per phase, so phase ph runs the item's pieces
// [ph NG, (ph + 1) NG). Longest first over the whole item, so the 16 row-groups of a wave get
// pieces of similar length. On entry out.items[i].w / out.ends[i] delimit item i's entries; on
// return its pieces. Also the dynamic-batch decision and the per-item / per-block statistics.
void build_pieces(const RbScheduleIn& in, RbScheduleOut& out) {
    const RbGeometry& g = in.geom;
    const Knobs& kn = *in.knobs;
    std::vector<RbItem>& items = out.items;
    std::vector<u32>& ends = out.ends;
    const u32 NT = g.NT, rowBytes = g.rowBytes;
    out.ient.resize(items.size());
    for (size_t i = 0; i < items.size(); ++i)
        out.ient[i] = RbPiece{items[i].w, (items[i].y == items[i].z && items[i].w == ends[i]) ? 0u
                                                                                          : ends[i] - items[i].w};
    // (per item on the host threads, then placed in item order)
    std::vector<std::vector<RbPiece>> ipc(items.size());
    par_for(items.size(), [&](unsigned, size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            std::vector<RbPiece>& mine = ipc[i];
            for_each_piece(in.entries, items[i].w, ends[i], kn.piece_max, [&](u32 e, u32 len, u32 col) {
                mine.push_back(RbPiece{e, col | ((len - 1) << 22)});
            });
            std::stable_sort(mine.begin(), mine.end(),
                             [](const RbPiece& a, const RbPiece& b) { return (a.y >> 22) > (b.y >> 22); });
        }
    }, 2048, in.threads);
    // dynamic piece batches (batches; kernels for rows of <= 512 B): after its first batch
    // of 64 / G pieces a wave takes the next from an LDS counter, which balances the waves of
    // items with several pieces per row-group. Measured (profiles/r05bt, forced on against off):
    // 512-byte rows with 2.4 / 6.5 / 6.8 pieces per row-group (mycielskian14 K = 128, C3, C4
    // x0.5) -4.5 / -2.4 / -2.2 %, C2's 1.4 +5 %; 128- and 256-byte rows (mycielskian15 K = 32,
    // Trefethen K = 64: little work per entry behind each counter round trip) +2 to +8 %. Auto:
    // 512-byte rows from batch_min_phases pieces per row-group
    {
        u64 npAll = 0;
        u32 nWork = 0;
        for (size_t i = 0; i < items.size(); ++i) {
            npAll += ipc[i].size();
            nWork += !(items[i].y == items[i].z && items[i].w == ends[i]);
        }
        const u32 NGl = NT / 4;  // row-groups (G = 4 for rows of <= 512 B)
        const double perItem = nWork ? static_cast<double>(npAll) / nWork : 0.0;
        out.dyn = rowBytes <= 512 &&
                  (kn.batches == 1 || (kn.batches < 0 && rowBytes == 512 && perItem >= kn.batch_min_phases * NGl));
    }
    // static phases (no batches): the item's pieces placed so that its waves end together
    // (balance_pieces; items with kept MFMA tiles keep the longest-first order, whose shortest
    // pieces sit with the tile waves)
    if (!out.dyn && kn.piece_balance == 1) {
        const u32 G = rowBytes >= 2048 ? 16 : rowBytes >= 1024 ? 8 : 4;  // rb_kernel.hpp RowGeom
        par_for(items.size(), [&](unsigned, size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; ++i)
                if (items[i].y == items[i].z) balance_pieces(ipc[i], NT, G, kn.piece_weight);
        }, 2048, in.threads);
    }
    std::vector<size_t> poff(items.size() + 1, 0);
    for (size_t i = 0; i < items.size(); ++i) poff[i + 1] = poff[i] + ipc[i].size();
    std::vector<RbPiece>& pieces = out.pieces;
    pieces.resize(poff.back());
    out.itemStat.assign(items.size(), RbItem{0, 0, 0, 0});
    std::vector<u64> ientc(items.size(), 0);
    std::vector<char> ipad(items.size(), 0);
    par_for(items.size(), [&](unsigned, size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            const bool pad = items[i].y == items[i].z && items[i].w == ends[i];
            std::copy(ipc[i].begin(), ipc[i].end(), pieces.begin() + poff[i]);
            std::vector<RbPiece>().swap(ipc[i]);
            items[i].w = static_cast<u32>(poff[i]);
            ends[i] = static_cast<u32>(poff[i + 1]);
            ipad[i] = pad;
            if (pad) continue;
            u64 ent = 0;
            for (u32 k = items[i].w; k < ends[i]; ++k) ent += (pieces[k].y >> 22) + 1;
            ientc[i] = ent;
            out.itemStat[i] = RbItem{items[i].x, items[i].z - items[i].y, static_cast<u32>(ent),
                                     ends[i] - items[i].w};
        }
    }, 2048, in.threads);
    out.rbCost.assign(g.nRB, 0.0);
    out.nWorkItems = 0;
    for (size_t i = 0; i < items.size(); ++i) {
        const RbItem it = items[i];
        if (ipad[i]) continue;  // padding
        ++out.nWorkItems;
        out.rbCost[it.x] += static_cast<double>(ientc[i]) + kn.shard_piece_weight * (ends[i] - it.w) +
                            16.0 * (it.z - it.y) + g.RB;
    }
}

}  // namespace

void rb_schedule(const RbScheduleIn& in, RbScheduleOut& out) {
    const auto lap = [&](const char* what) {
        if (in.lap) in.lap(what);
    };
    const u32 NCR = RB_XCDS * in.geom.m;
    const std::vector<u32> cuts = column_cuts(in, NCR);
    lap("cuts");
    const Segments seg = build_segments(in, cuts, NCR);
    lap("segments");
    const Lists lists = ChunkPlanner(in, seg).plan();
    lap("chunks");
    interleave(lists, in.geom.staged, out.items, out.ends);
    lap("items");
    build_pieces(in, out);
    lap("pieces");
}

namespace {
// the runs of one item's sorted positions pos[0, len): written to dst unless null; their number
u32 runs_of(const u32* pos, u32 len, RbPiece* dst) {
    u32 nrun = 0;
    for (u32 t = 0; t < len;) {
        u32 u = t + 1;
        while (u < len && u - t < RB_RUN_MAX && pos[u] == pos[u - 1] + 1) ++u;
        if (dst) dst[nrun] = RbPiece{pos[t], t | ((u - t) << 16)};
        ++nrun;
        t = u;
    }
    return nrun;
}
}  // namespace

void rb_cut_runs(const u32* sortedPos, const RbPiece* ient, size_t nItems, u32 NT, RbRuns& out, unsigned threads) {
    // two passes on the host threads: count each item's runs, then (offsets by a scan) write them
    // in item order into one flat table (no per-item vectors: C4 x1 holds ~60 M runs)
    out.itemRuns.assign(nItems, RbPiece{0, 0});
    par_for(nItems, [&](unsigned, size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) out.itemRuns[i].y = runs_of(sortedPos + ient[i].x, ient[i].y, nullptr);
    }, 2048, threads);
    out.fits = true;
    size_t nr = 0;
    for (size_t i = 0; i < nItems; ++i) {
        out.fits = out.fits && out.itemRuns[i].y <= NT;
        out.itemRuns[i].x = static_cast<u32>(nr);
        nr += out.itemRuns[i].y;
    }
    out.runs.assign(out.fits ? nr : 0, RbPiece{0, 0});
    if (out.fits)
        par_for(nItems, [&](unsigned, size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; ++i)
                runs_of(sortedPos + ient[i].x, ient[i].y, out.runs.data() + out.itemRuns[i].x);
        }, 2048, threads);
}

}  // namespace bsmr
