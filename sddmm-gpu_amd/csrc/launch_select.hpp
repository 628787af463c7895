// launch_select.hpp — which launch bsmr_sddmm runs for (K, dtype), which form of the row-block
// kernel a layout takes, and the argument rules of the launch entry points: every such decision,
// once. Standard library only: no HIP, no device, so it builds, runs and is tested on a machine
// without a GPU. The rules read a few plain numbers (PlanFacts, RbLayoutFacts) that plan.hpp fills
// from a Plan, and the plan's tuning (knobs.hpp Knobs) beside them; sddmm.hip, plan_check.cpp,
// spmm.hip and capi.cpp ask here and never restate a rule. A success costs a few compares:
// messages are built on the error path only.
#pragma once

#include <cstdint>
#include <string>

#include "verdict.hpp"

namespace bsmr {

struct Knobs;  // knobs.hpp

// the values of bsmr.h that the rules use (plan.hpp asserts that they agree)
constexpr int LS_F32 = 0, LS_F16 = 1, LS_BF16 = 2;
constexpr int LS_OK = 0, LS_ERR_INVALID = 1, LS_ERR_UNSUPPORTED = 6;
constexpr uint32_t LS_XCDS = 8;  // XCD_BUCKETS (plan.hpp)

// what the launch decision reads from a Plan (plan.hpp launch_facts) beside its Knobs; the fields
// are documented at Plan's members of the same name
struct PlanFacts {
    uint32_t M = 0, N = 0, nnz = 0, nres = 0, numDenseTiles = 0;
};

// the residual carries under a quarter of the work (a tile ~ 16 entries): 16 x 16 block masks
bool tile_dominated(const PlanFacts& f);
// (K, dtype) -> row-block layout slot by row bytes (0..4: 128 B .. 2 KiB); -1: no row-block launch
int rb_slot(const PlanFacts& f, const Knobs& k, uint32_t K, int dtype);
// whether the whole-plan row-block launch of rows of rowBytes builds the column-block candidate
// (Knobs::col_blocks: 1 always, 2 for wide patterns N >= 2 M, else never). The candidate gathers A
// rows the way the plain launch gathers B rows, so it exists only when M <= 2^22 and M rowBytes <
// 2^32; otherwise it is skipped, for col_blocks = 1 too, and the launch runs the row-block layout
// already built. bsmr_debug_col_block_candidate reports the value
bool col_block_candidate(const PlanFacts& f, const Knobs& k, uint32_t rowBytes);
// fp16/bf16 patterns dense enough for whole MFMA tiles (sddmm_dense.hip); asked after use_ptile
bool use_dense(const PlanFacts& f, const Knobs& k, uint32_t K, int dtype);
// tile-dominated fp16/bf16 plans with K in {64, 128, 256, 512}: the panel-grouped tile launch
bool use_ptile(const PlanFacts& f, const Knobs& k, uint32_t K, int dtype);

// the launch bsmr_sddmm / bsmr_sddmm_batch runs for (K, dtype); bsmr_debug_launch_choice reports
// the values
enum class Launch : uint32_t { Ptile = 0, Dense = 1, RowBlock = 2, Half = 3, ColMajor = 4 };
struct LaunchChoice {
    Launch kind = Launch::ColMajor;
    // rb_slot, whatever the kind: the panel entry points and the shard cuts run row blocks on
    // plans whose whole launch is another
    int slot = -1;
    uint32_t rowBytes = 0;  // K * the operands' element size
};
LaunchChoice choose_launch(const PlanFacts& f, const Knobs& k, uint32_t K, int dtype);

// what the form of a row-block launch reads from its layout (Plan::RowBlockLayout's members of the
// same name; plan.hpp rb_layout_facts)
struct RbLayoutFacts {
    uint32_t rowBytes = 0, NT = 1024, nItems = 0, nTilesKept = 0, outLds = 0;
    bool outRuns = false, dynBatches = false;
};
// the kernel form and launch configuration of a row-block launch (sddmm.hip launch_rb, pick_rb)
struct RbForm {
    bool stageNt = false;  // the A rows staged with the nt policy
    bool lateB = true;     // phase-0 B loads after the staging barrier
    bool pairs = false;    // k_sddmm_rb_pair: two items per workgroup
    bool lite = false;     // the LITE single-item kernel
    bool dyn = false;      // dynamic piece batches
    uint32_t NT = 1024, grid = 0, ldsBytes = 0;
    // 1 KiB blocks of the launch's LDS that the staging fills; 0: the blocks of the A image (rows
    // per block x row bytes, the layout's own geometry)
    uint32_t stageBlocks = 0;
};
// mode: 1 = dense tiles only, 2 = residual only, 3 = both (the whole launch)
RbForm rb_form(const RbLayoutFacts& L, const Knobs& k, uint32_t mode);

// K / dtype rules of every launch and prepare call, reported under the caller's name
Verdict validate_kd(const char* who, uint32_t K, int dtype);
// the further K rule of the launch chosen: the half column-major launch takes multiples of 32,
// the panel-tile launch K in {64, 128, 256, 512}
Verdict validate_launch_k(const char* who, Launch kind, uint32_t K);
// the panel-range rules of bsmr_sddmm_panels / _panels_local and their prepare calls: [p0, p1)
// within the plan's P panels; a non-empty range needs a row-block slot when the A rows are local
// or the operands fp16/bf16 (fp32 falls back to the panel-major lists)
Verdict check_panel_range(const char* who, uint32_t p0, uint32_t p1, uint32_t P, int slot, int dtype,
                          bool local);

}  // namespace bsmr
