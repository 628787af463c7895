// launch_select.cpp — the launch decision of bsmr_sddmm (launch_select.hpp). Host only.
#include "launch_select.hpp"

#include <cstring>

#include "knobs.hpp"

namespace bsmr {

bool tile_dominated(const PlanFacts& f) {
    return static_cast<uint64_t>(f.nres) * 4 < static_cast<uint64_t>(f.numDenseTiles) * 16;
}

int rb_slot(const PlanFacts& f, const Knobs& k, uint32_t K, int dtype) {
    if (f.N > (1u << 22) || !k.use_rowblock) return -1;
    // tile-dominated plans (e.g. 16x16 block masks): one tile per wave with A from L2 beats
    // staging row blocks (C5 block mask: 8.9 vs 11.1 us); row blocks pay off once the residual
    // carries a quarter of the work (a tile ~ 16 entries)
    if (!k.force_rowblock && tile_dominated(f)) return -1;
    const uint32_t rby = K * (dtype == LS_F32 ? 4u : 2u);
    // the row-block kernel addresses B with 32-bit byte offsets (load_bcol): B < 4 GiB
    if (static_cast<uint64_t>(f.N) * rby >= (1ull << 32)) return -1;
    return rby == 128 ? 0 : rby == 256 ? 1 : rby == 512 ? 2 : rby == 1024 ? 3 : rby == 2048 ? 4 : -1;
}

bool col_block_candidate(const PlanFacts& f, const Knobs& k, uint32_t rowBytes) {
    if (k.col_blocks != 1 && !(k.col_blocks == 2 && static_cast<uint64_t>(f.N) >= 2ull * f.M)) return false;
    // the roles swapped, A's rows are the gathered ones: the metadata's 22-bit "column" holds an
    // original row, and load_bcol's 32-bit byte offset runs over A. (Under rule 2 both follow from
    // rb_slot: N >= 2 M, N <= 2^22 and N rowBytes < 2^32.)
    return f.M <= (1u << 22) && static_cast<uint64_t>(f.M) * rowBytes < (1ull << 32);
}

bool use_dense(const PlanFacts& f, const Knobs& k, uint32_t K, int dtype) {
    // layout auto only (BSMR_LAYOUT_ROWBLOCK / _COLMAJOR force those launches); choose_launch asks
    // use_ptile first (tile-dominated fp16/bf16 plans, K in {64..512}: C5 block 7.8 -> 5.6 us)
    // tile-dominated plans (16 x 16 block masks) keep the column-major tile launch below K = 512:
    // a 128 x 128 tile's fixed prologue and epilogue only pay off over long K (C5 block mask,
    // bf16: dense 8.2 vs 8.9 us at K = 512, 5.95 vs 5.35 at 256, 4.7 vs 3.8 at 128;
    // profiles/r02c/dense_blockmask_ab.txt)
    if (K < 512 && tile_dominated(f)) return false;
    return k.use_rowblock && !k.force_rowblock && dtype != LS_F32 && K % 64 == 0 &&
           static_cast<double>(f.nnz) >= static_cast<double>(k.dense_min) * f.M * static_cast<double>(f.N);
}

// every BSMR tile on MFMA with the panel's A rows staged once per item (sddmm_half.hip
// k_sddmm_ptile; BSMR_PTILE = 1: whenever the dtype and K allow, also beside a large residual; 0:
// never)
bool use_ptile(const PlanFacts& f, const Knobs& k, uint32_t K, int dtype) {
    if (dtype == LS_F32 || k.ptile_mode == 0 || !k.use_rowblock || k.force_rowblock) return false;
    if ((K != 64 && K != 128 && K != 256 && K != 512) || f.numDenseTiles == 0) return false;
    return k.ptile_mode == 1 || tile_dominated(f);
}

LaunchChoice choose_launch(const PlanFacts& f, const Knobs& k, uint32_t K, int dtype) {
    LaunchChoice c;
    c.rowBytes = K * (dtype == LS_F32 ? 4u : 2u);
    c.slot = rb_slot(f, k, K, dtype);
    c.kind = use_ptile(f, k, K, dtype)   ? Launch::Ptile
             : use_dense(f, k, K, dtype) ? Launch::Dense
             : c.slot >= 0            ? Launch::RowBlock
             : dtype != LS_F32        ? Launch::Half
                                      : Launch::ColMajor;
    return c;
}

RbForm rb_form(const RbLayoutFacts& L, const Knobs& k, uint32_t mode) {
    RbForm f;
    f.stageNt = k.stage_nt == 1;
    f.lateB = k.late_b != 0;
    // pairs (BSMR_DIAG & 16384 off): the whole launch, staged output by runs, rows of >= 512
    // bytes, at least pair_min_items (4096: 16 rounds of the chip's workgroup slots) items, an even
    // number of list positions per XCD, no kept MFMA tile; not under the profiling ablations
    // (trace, staging only, B in L2, no stores) nor nt staging / early B loads. A pair is two
    // items long, so short lists lose to the tail: mycielskian15 K = 64 / 128 (832 / 728 items)
    // 56.9 / 74.6 us paired against 50.1 / 66.5 unpaired, mycielskian16 K = 64 114.6 against
    // 108.9; C4 (8-30 K items) gains (x0.5 1.029 -> 0.984 ms), C3, mycielskian16 K = 128 and
    // 1-2 KiB rows are neutral (profiles/r04zt, r04zw)
    f.pairs = mode == 3 && L.outRuns && L.outLds && L.rowBytes >= 512 && L.nItems >= k.pair_min_items &&
              L.nTilesKept == 0 && L.nItems % (2 * LS_XCDS) == 0 && !f.stageNt && f.lateB &&
              !(k.diag & (8u | 32u | 64u | 128u | 16384u));
    // the LITE single-item kernel: the whole launch (mode 3), no kept tiles, direct stores, default
    // staging policy, late B, no trace or ablation bits (BSMR_DIAG & 33554432 keeps the full form
    // for A/B)
    f.lite = mode == 3 && L.nTilesKept == 0 && !L.outLds && !f.stageNt && f.lateB && k.diag == 0;
    f.dyn = L.dynBatches;
    f.NT = L.NT;
    f.grid = f.pairs ? L.nItems / 2 : L.nItems;
    // the workgroup's LDS: 160 / 80 KiB (the image, the staged-output slots, the batch counter)
    f.ldsBytes = (L.NT == 1024 ? 160u : 80u) * 1024u;
    // the image's blocks only (BSMR_DIAG & 2097152, A/B only: every block of the launch's LDS but
    // the last, which holds the piece-batch counter — the filler past the image reading row 0, as
    // before round 5)
    f.stageBlocks = (k.diag & 2097152u) ? (L.NT == 1024 ? 159u : 79u) : 0u;
    return f;
}

Verdict validate_kd(const char* who, uint32_t K, int dtype) {
    if (K == 0 || K % 16 != 0)
        return {LS_ERR_UNSUPPORTED, std::string(who) + ": K must be a positive multiple of 16"};
    if (dtype != LS_F32 && dtype != LS_F16 && dtype != LS_BF16)
        return {LS_ERR_UNSUPPORTED, std::string(who) + ": dtype must be BSMR_F32, BSMR_F16 or BSMR_BF16"};
    return {};
}

Verdict validate_launch_k(const char* who, Launch kind, uint32_t K) {
    if (kind == Launch::Half && (K == 0 || K % 32 != 0))
        return {LS_ERR_UNSUPPORTED,
                std::string(who) + ": fp16/bf16 inputs need K to be a positive multiple of 32"};
    if (kind == Launch::Ptile && K != 64 && K != 128 && K != 256 && K != 512)
        return {LS_ERR_UNSUPPORTED,
                std::string(who) + ": the panel-tile launch needs K in {64, 128, 256, 512}"};
    return {};
}

Verdict check_panel_range(const char* who, uint32_t p0, uint32_t p1, uint32_t P, int slot, int dtype,
                          bool local) {
    if (p0 > p1 || p1 > P) return {LS_ERR_INVALID, std::string(who) + ": bad panel range"};
    if (p0 == p1 || slot >= 0) return {};
    if (local)  // (the prepare calls name the launch they prepare)
        return {LS_ERR_UNSUPPORTED,
                std::string(who) +
                    (std::strcmp(who, "bsmr_sddmm_panels_local") ? ": bsmr_sddmm_panels_local needs" : ": needs") +
                    " the row-block launch (rows of 128 B .. 2 KiB)"};
    if (dtype != LS_F32)
        return {LS_ERR_UNSUPPORTED,
                std::string(who) + ": fp16/bf16 panel ranges need the row-block layout (half K in 128..1024)"};
    return {};
}

}  // namespace bsmr
