// panel_host.hpp — what the panel families share on the host (attention_panels.hip and its e4m3
// form, attention_bwd_panels.hip, spmm_panels.hip, sddmm_panels.hip): the plan's two panel lists
// (Plan::PanelListState) and their upload, the list counters of a stats record, the argument rules
// of the attention families, the build of missing state at a launch and the launches themselves.
#pragma once

#include <string>

#include "attention_common.hpp"
#include "attention_panels.hpp"
#include "panel_mfma.hpp"
#include "plan.hpp"

namespace bsmr {

// panel_rows (once): attention_panel_lists over the plan's CSR in the plan's reordered row order;
// layout_mu held. Synchronous on the plan's stream. `who` names the caller in errors. Defined in
// attention_panels.hip
int attn_panels_build_lists(const Plan& p, const char* who);
// panel_cols (once): attention_panel_lists on the transposed pattern, M and N in each other's role
// and no order, so a column panel is 16 consecutive columns. Defined in attention_bwd_panels.hip
int attn_bwd_panels_build_col_lists(const Plan& p, const char* who);

// A side's lists (1 rows, 2 columns: through the builder above when they are not built) and, once,
// where in the caller's nnz-sized vector the entry of every set mask bit lies (SpmmPanelsSide's base
// and pos, spmm_panels.hpp) with stepWaves; no scratch. layout_mu held; synchronous on the plan's
// stream. The panel SpMM's sides and the MFMA SDDMM (sddmm_panels.hip, side 1) build through it.
// Defined in spmm_panels.hip
int spmm_panels_build_positions(const Plan& p, int side, const char* who);

// What attention_panel_lists returned (st, err, L) into S: its faults mapped (2, past the lists'
// capacity, and more than 2^31 items are BSMR_ERR_UNSUPPORTED), the four arrays uploaded, the
// plan's stream synchronised, the counters set. Defined in attention_panels.hip
int panel_lists_upload(const Plan& p, Plan::PanelListState& S, int st, const std::string& err, const PanelLists& L,
                       const char* who);

// the six list counters of a stats record
inline void panel_list_stats(const Plan::PanelListState& S, u64 nnz, u32& panels, u32& items, u32& steps, u32& split_panels,
                             u32& partials, u32& fill_permille) {
    panels = S.panels;
    items = S.nItems;
    steps = S.nSteps;
    split_panels = S.splitPanels;
    partials = S.partials;
    fill_permille = panel_fill_permille(nnz, S.nSteps);
}

// fp16 / bf16 and D and Dv each one of the compile-time forms, 32, 64, 128 and, `with256`, 256; else
// BSMR_ERR_UNSUPPORTED with the message set. Defined in attention_panels.hip
int panel_validate_dims(const char* who, u32 D, u32 Dv, int dtype, bool with256);
// a prepare or prepared call's arguments (they carry no dtype)
int panel_prepare_args(const char* who, const bsmr_plan* plan, u32 D, u32 Dv, u32 slices, bool with256);

// At a launch, layout_mu held: what `ready` misses is built by `build`, unless the stream is
// capturing: then BSMR_ERR_NOT_PREPARED, and the message names what `missing` returns
template <class Ready, class Missing, class Build>
int panel_build_missing(const LaunchSite& at, Ready ready, Missing missing, Build build) {
    if (ready()) return BSMR_OK;
    const int st = lazy_build_guard(at);
    if (st == BSMR_ERR_NOT_PREPARED)
        set_error(std::string(at.who) + ": stream is capturing and " + missing() + " are not built; call " + at.prep + " first");
    BSMR_CHECK(st);
    return build();
}
inline std::string panel_slices_clause(u32 slices) { return slices > 1 ? ", " + std::to_string(slices) + " slices" : std::string(); }

// `fn` over the items in workgroups of PANEL_WAVES waves, then `red` over the split panels, one
// thread per row and four of the 4 q4 columns; `outer` and `redOuter` are the grids' y and z
template <class Args, class... Extra>
int panel_launch(hipStream_t s, void (*fn)(const Args), const Args& a, u32 nItems, dim3 outer,
                 void (*red)(const Args, const PanelRed*, u32, Extra...), const PanelRed* reds, u32 nReds, u32 q4, dim3 redOuter,
                 Extra... extra) {
    if (nItems) {
        outer.x = (nItems + PANEL_WAVES - 1) / PANEL_WAVES;
        hipLaunchKernelGGL(fn, outer, dim3(PANEL_WAVES * 64), 0, s, a);
        BSMR_HIP(hipGetLastError());
    }
    if (nReds) {
        const size_t threads = static_cast<size_t>(nReds) * PANEL_ROWS * q4;
        redOuter.x = static_cast<u32>((threads + 255) / 256);
        hipLaunchKernelGGL(red, redOuter, dim3(256), 0, s, a, reds, nReds, extra...);
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

}  // namespace bsmr
