// knobs.cpp — defaults, environment parser and apply rules of the plan's tuning (knobs.hpp). Host only.
#include "knobs.hpp"

#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <string>
#include <type_traits>

namespace {

// Every field of bsmr_tuning, in the header's order, with how its BSMR_<FIELD> variable parses:
// INT atoi, FLT atof, TRI a tri-state switch ("0" never, "1" always, anything else auto)
enum Kind { INT, TRI, FLT };
#define BSMR_TUNING_FIELDS(X)                                                                        \
    X(diag, INT) X(tile_min_f32, INT) X(tile_min_half, INT) X(piece_max, INT) X(piece_weight, FLT)   \
    X(shard_piece_weight, FLT) X(dense_min, FLT) X(orig_rows, TRI) X(orig_contig, INT)               \
    X(dense_ks, INT) X(dense_ns, INT) X(out_staged, TRI) X(l2_range_kb, INT) X(stage_nt, TRI)        \
    X(rb_rows, INT) X(late_b, INT) X(item_cap, FLT) X(item_sched, TRI) X(out_packed, TRI)            \
    X(cluster_filter, TRI) X(pair_min_items, INT) X(batches, TRI) X(ptile, TRI) X(ptile_tpi, INT)    \
    X(piece_balance, TRI) X(col_blocks, INT)

#define X(name, kind) +1
static_assert((0 BSMR_TUNING_FIELDS(X)) * 4 == sizeof(bsmr_tuning),
              "a field of bsmr_tuning is missing from BSMR_TUNING_FIELDS");
#undef X
// (parse and set_auto below go by the field's C type: a row's kind has to be that type's)
template <class T>
constexpr bool kind_fits(Kind kind) {
    return std::is_same<T, float>::value ? kind == FLT : std::is_same<T, int32_t>::value ? kind != FLT : kind == INT;
}
#define X(name, kind) \
    static_assert(kind_fits<decltype(bsmr_tuning::name)>(kind), "BSMR_TUNING_FIELDS: kind of " #name);
BSMR_TUNING_FIELDS(X)
#undef X

// "auto": -1, or < 0 for the floats; the one unsigned field (diag) 0
void set_auto(uint32_t& f) { f = 0; }
void set_auto(int32_t& f) { f = -1; }
void set_auto(float& f) { f = -1.0f; }

void parse(Kind, const char* v, uint32_t& f) { f = static_cast<uint32_t>(std::atoi(v)); }
void parse(Kind kind, const char* v, int32_t& f) {
    f = kind == TRI ? (v[0] == '0' ? 0 : v[0] == '1' ? 1 : -1) : std::atoi(v);
}
void parse(Kind, const char* v, float& f) { f = static_cast<float>(std::atof(v)); }

// the field's variable, "BSMR_" + its name in upper case, when set
template <class T>
int from_env(const char* field, Kind kind, T& f) {
    std::string name = "BSMR_";
    for (const char* c = field; *c; ++c) name += static_cast<char>(std::toupper(static_cast<unsigned char>(*c)));
    const char* v = std::getenv(name.c_str());
    if (v) parse(kind, v, f);
    return v != nullptr;
}

}  // namespace

extern "C" void bsmr_plan_options_default(bsmr_plan_options* o) {
    o->alpha = 0.3f;   // Options.hpp:40
    o->delta = 0.3f;   // Options.hpp:41
    o->free_mem_bytes = 0;
    o->device = 0;
    o->cluster_batch = 0;
    o->exact_similarity = 0;
    o->layout = BSMR_LAYOUT_AUTO;
    o->lds_budget_kb = 0;
    o->tuning = nullptr;
}

extern "C" void bsmr_tuning_default(bsmr_tuning* t) {
#define X(name, kind) set_auto(t->name);
    BSMR_TUNING_FIELDS(X)
#undef X
}

extern "C" int bsmr_tuning_from_env(bsmr_tuning* t) {
    int n = 0;
#define X(name, kind) n += from_env(#name, kind, t->name);
    BSMR_TUNING_FIELDS(X)
#undef X
    return n;
}

namespace bsmr {

void apply_tuning(Knobs& k, const bsmr_tuning& t) {
    k.diag = t.diag;
    if (t.tile_min_f32 >= 0) k.tile_min_f32 = static_cast<uint32_t>(t.tile_min_f32);
    if (t.tile_min_half >= 0) k.tile_min_half = static_cast<uint32_t>(t.tile_min_half);
    if (t.piece_max >= 0) k.piece_max = std::min<uint32_t>(RB_PIECE_MAX, std::max(1, t.piece_max));
    if (t.piece_weight >= 0) k.piece_weight = t.piece_weight;
    if (t.shard_piece_weight >= 0) k.shard_piece_weight = t.shard_piece_weight;
    if (t.dense_min >= 0) k.dense_min = t.dense_min;
    if (t.orig_rows >= 0) k.orig_rows = t.orig_rows ? 1 : 0;
    if (t.orig_contig >= 0) k.orig_contig = t.orig_contig;
    if (t.dense_ks >= 0) k.dense_ks = t.dense_ks;
    if (t.dense_ns >= 0) k.dense_ns = t.dense_ns;
    if (t.out_staged >= 0) k.out_staged = t.out_staged ? 1 : 0;
    if (t.out_packed >= 0) k.out_packed = t.out_packed ? 1 : 0;
    if (t.stage_nt >= 0) k.stage_nt = t.stage_nt ? 1 : 0;
    if (t.rb_rows > 0) k.rb_rows_force = t.rb_rows;
    if (t.late_b >= 0) k.late_b = t.late_b;
    if (t.item_cap >= 0) k.item_cap = t.item_cap;
    if (t.item_sched >= 0)
        k.item_cost_cuts = k.item_lpt = k.small_sparse_rb = t.item_sched != 0;
    if (t.cluster_filter >= 0) k.cluster_filter = t.cluster_filter ? 1 : 0;
    if (t.pair_min_items >= 0) k.pair_min_items = static_cast<uint32_t>(t.pair_min_items);
    if (t.batches >= 0) k.batches = t.batches ? 1 : 0;
    if (t.ptile >= 0) k.ptile_mode = t.ptile ? 1 : 0;
    if (t.ptile_tpi >= 0) k.ptile_tpi = static_cast<uint32_t>(std::min(64, t.ptile_tpi));
    if (t.piece_balance >= 0) k.piece_balance = t.piece_balance ? 1 : 0;
    if (t.col_blocks >= 0) k.col_blocks = std::min(2, t.col_blocks);
    if (t.l2_range_kb >= 0) {
        k.l2_range_kb = static_cast<uint32_t>(std::max(64, t.l2_range_kb));
        k.l2_range_user = true;
    }
}

Verdict apply_options(Knobs& k, const bsmr_plan_options& o) {
    if (o.cluster_batch) k.cluster_batch = o.cluster_batch;
    if (o.layout < BSMR_LAYOUT_AUTO || o.layout > BSMR_LAYOUT_COLMAJOR ||
        (o.lds_budget_kb && (o.lds_budget_kb < 16 || o.lds_budget_kb > 160)))
        return {BSMR_ERR_INVALID, "bsmr_plan: bad layout or lds_budget_kb"};
    k.use_rowblock = o.layout != BSMR_LAYOUT_COLMAJOR;
    k.force_rowblock = o.layout == BSMR_LAYOUT_ROWBLOCK;
    if (o.lds_budget_kb) {
        k.rb_lds_kb = o.lds_budget_kb;
        k.rb_lds_user = true;
    }
    if (o.tuning) apply_tuning(k, *o.tuning);
    return {};
}

}  // namespace bsmr
