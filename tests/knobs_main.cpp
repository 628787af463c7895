// Stand-alone driver of the host-only tuning unit (csrc/knobs.cpp), built by
// tests/test_knobs_cpu.py under -fsanitize=address,undefined with no HIP include path.
//   knobs_main apply <file>: every line of the file holds the 26 fields of bsmr_tuning in the
//     header's order, then layout, lds_budget_kb and cluster_batch; prints one line per row, "code
//     <status> name value ... | <message>", with every member of Knobs after apply_options.
//   knobs_main env: bsmr_tuning_default and bsmr_tuning_from_env on every field, its variable set
//     by this program; prints "env ok <fields>" or the first difference (exit status 3).
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "knobs.hpp"

namespace {

// the fields as include/bsmr.h documents them: variable, kind (u unsigned, i int, t tri-state,
// f float), place in the struct
struct Field {
    const char* env;
    char kind;
    size_t off;
};
#define F(env, kind, name) {env, kind, offsetof(bsmr_tuning, name)}
const Field FIELDS[] = {
    F("BSMR_DIAG", 'u', diag), F("BSMR_TILE_MIN_F32", 'i', tile_min_f32), F("BSMR_TILE_MIN_HALF", 'i', tile_min_half),
    F("BSMR_PIECE_MAX", 'i', piece_max), F("BSMR_PIECE_WEIGHT", 'f', piece_weight),
    F("BSMR_SHARD_PIECE_WEIGHT", 'f', shard_piece_weight), F("BSMR_DENSE_MIN", 'f', dense_min),
    F("BSMR_ORIG_ROWS", 't', orig_rows), F("BSMR_ORIG_CONTIG", 'i', orig_contig), F("BSMR_DENSE_KS", 'i', dense_ks),
    F("BSMR_DENSE_NS", 'i', dense_ns), F("BSMR_OUT_STAGED", 't', out_staged), F("BSMR_L2_RANGE_KB", 'i', l2_range_kb),
    F("BSMR_STAGE_NT", 't', stage_nt), F("BSMR_RB_ROWS", 'i', rb_rows), F("BSMR_LATE_B", 'i', late_b),
    F("BSMR_ITEM_CAP", 'f', item_cap), F("BSMR_ITEM_SCHED", 't', item_sched), F("BSMR_OUT_PACKED", 't', out_packed),
    F("BSMR_CLUSTER_FILTER", 't', cluster_filter), F("BSMR_PAIR_MIN_ITEMS", 'i', pair_min_items),
    F("BSMR_BATCHES", 't', batches), F("BSMR_PTILE", 't', ptile), F("BSMR_PTILE_TPI", 'i', ptile_tpi),
    F("BSMR_PIECE_BALANCE", 't', piece_balance), F("BSMR_COL_BLOCKS", 'i', col_blocks)};
#undef F
constexpr size_t NF = sizeof(FIELDS) / sizeof(FIELDS[0]);
static_assert(NF == 26 && NF * 4 == sizeof(bsmr_tuning), "every field of bsmr_tuning");

// a field's value as a double (every value the tests use is exact in all three types)
double get(const bsmr_tuning& t, const Field& f) {
    const char* p = reinterpret_cast<const char*>(&t) + f.off;
    if (f.kind == 'f') {
        float v;
        memcpy(&v, p, 4);
        return v;
    }
    if (f.kind == 'u') {
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    }
    int32_t v;
    memcpy(&v, p, 4);
    return v;
}
void put(bsmr_tuning& t, const Field& f, double x) {
    char* p = reinterpret_cast<char*>(&t) + f.off;
    if (f.kind == 'f') {
        const float v = static_cast<float>(x);
        memcpy(p, &v, 4);
    } else if (f.kind == 'u') {
        const uint32_t v = static_cast<uint32_t>(x);
        memcpy(p, &v, 4);
    } else {
        const int32_t v = static_cast<int32_t>(x);
        memcpy(p, &v, 4);
    }
}

int apply(const char* path) {
    FILE* in = fopen(path, "r");
    if (!in) return 2;
    for (;;) {
        bsmr_tuning t;
        double x;
        size_t i = 0;
        for (; i < NF && fscanf(in, "%lf", &x) == 1; ++i) put(t, FIELDS[i], x);
        if (i == 0) break;
        bsmr_plan_options o;
        bsmr_plan_options_default(&o);
        if (i != NF || fscanf(in, "%d %" SCNu32 " %" SCNu32, &o.layout, &o.lds_budget_kb, &o.cluster_batch) != 3) return 2;
        o.tuning = &t;
        bsmr::Knobs k;
        const bsmr::Verdict v = bsmr::apply_options(k, o);
        printf("code %d", v.code);
#define B(name) printf(" " #name " %d", k.name ? 1 : 0);
#define I(name) printf(" " #name " %lld", static_cast<long long>(k.name));
#define D(name) printf(" " #name " %.9g", static_cast<double>(k.name));
        B(use_rowblock) B(force_rowblock) I(rb_lds_kb) B(rb_lds_user) I(rb_lds_kb_staged) I(l2_range_kb_staged)
        I(diag) I(l2_range_kb) B(l2_range_user) I(piece_max) D(piece_weight) D(shard_piece_weight)
        I(out_staged) I(out_packed) I(stage_nt) I(rb_rows_force) I(late_b) D(item_cap) B(item_cost_cuts)
        B(item_lpt) D(item_fixed) B(small_sparse_rb) I(out_staged_min) D(dense_min) I(cluster_batch)
        I(cluster_filter) I(filter_min_rows) I(pair_min_items) I(batches) D(batch_min_phases) I(piece_balance)
        I(orig_rows) I(col_blocks) I(orig_contig) I(tile_min_f32) I(tile_min_half) I(dense_ks) I(dense_ns)
        I(ptile_mode) I(ptile_tpi)
#undef B
#undef I
#undef D
        printf(" | %s\n", v.msg.c_str());
    }
    fclose(in);
    return 0;
}

#define WANT(cond, ...)           \
    if (!(cond)) {                \
        printf(__VA_ARGS__);      \
        printf("\n");             \
        return 3;                 \
    }

// from_env on a struct filled with 77 after `text` went to field i's variable alone: `count`
// fields taken, field i = want, every other field untouched
int env_case(size_t i, const char* text, double want) {
    for (const Field& f : FIELDS) unsetenv(f.env);
    setenv(FIELDS[i].env, text, 1);
    bsmr_tuning t;
    for (const Field& f : FIELDS) put(t, f, 77);
    const int n = bsmr_tuning_from_env(&t);
    WANT(n == 1, "%s=%s: %d fields taken", FIELDS[i].env, text, n);
    for (size_t j = 0; j < NF; ++j)
        WANT(get(t, FIELDS[j]) == (j == i ? want : 77.0), "%s=%s: field %s = %g", FIELDS[i].env, text, FIELDS[j].env,
             get(t, FIELDS[j]));
    return 0;
}

int env() {
    for (const Field& f : FIELDS) unsetenv(f.env);
    bsmr_tuning t;
    memset(&t, 0x5a, sizeof(t));
    bsmr_tuning_default(&t);
    for (const Field& f : FIELDS)  // "auto": -1, < 0 for the floats, diag 0
        WANT(get(t, f) == (f.kind == 'u' ? 0.0 : -1.0), "default of %s = %g", f.env, get(t, f));
    WANT(bsmr_tuning_from_env(&t) == 0, "a field taken from an empty environment");
    for (const Field& f : FIELDS) WANT(get(t, f) == (f.kind == 'u' ? 0.0 : -1.0), "%s touched", f.env);
    for (size_t i = 0; i < NF; ++i) {
        int bad = 0;
        switch (FIELDS[i].kind) {
            case 'u':  // atoi into the unsigned field
                bad = env_case(i, "8", 8) || env_case(i, "2097152", 2097152) || env_case(i, "x", 0);
                break;
            case 'i':  // atoi
                bad = env_case(i, "3", 3) || env_case(i, "-7", -7) || env_case(i, "0", 0) || env_case(i, "12abc", 12) ||
                      env_case(i, "abc", 0) || env_case(i, "", 0);
                break;
            case 't':  // by the first character: '0' -> 0, '1' -> 1, anything else -> -1
                bad = env_case(i, "0", 0) || env_case(i, "1", 1) || env_case(i, "17", 1) || env_case(i, "03", 0) ||
                      env_case(i, "2", -1) || env_case(i, "auto", -1) || env_case(i, "-1", -1) || env_case(i, "", -1);
                break;
            default:  // atof
                bad = env_case(i, "2.5", 2.5) || env_case(i, "-1", -1) || env_case(i, "0", 0) || env_case(i, "1e-3", 1e-3f) ||
                      env_case(i, "x", 0);
        }
        if (bad) return bad;
    }
    // all at once
    for (const Field& f : FIELDS) setenv(f.env, f.kind == 'f' ? "0.25" : f.kind == 't' ? "1" : "5", 1);
    bsmr_tuning_default(&t);
    const int n = bsmr_tuning_from_env(&t);
    WANT(n == static_cast<int>(NF), "%d of %zu fields taken", n, NF);
    for (const Field& f : FIELDS)
        WANT(get(t, f) == (f.kind == 'f' ? 0.25 : f.kind == 't' ? 1.0 : 5.0), "all set: %s = %g", f.env, get(t, f));
    printf("env ok %zu\n", NF);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "apply")) return apply(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "env")) return env();
    fprintf(stderr, "usage: %s apply <file> | env\n", argv[0]);
    return 2;
}
