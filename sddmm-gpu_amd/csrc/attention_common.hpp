// attention_common.hpp — what the fused attention forward (attention.hip) and backward
// (attention_bwd.hip) share on the host: the argument rules and the rows' segment lists. One copy,
// defined in attention.hip, so that the two entry points cannot drift apart.
#pragma once

#include <string>

#include "plan.hpp"
#include "spmm_schedule.hpp"

namespace bsmr {

constexpr u32 ATTN_MAX_ROW_BYTES = 1024;

// D a positive multiple of 16 (fp32) or 32 (fp16 / bf16), Dv of 16, rows of at most
// ATTN_MAX_ROW_BYTES bytes, a known dtype; else BSMR_ERR_UNSUPPORTED with the message set
int attn_validate_dims(const char* who, u32 D, u32 Dv, int dtype);
// the prepare calls carry no dtype: what some dtype accepts
int attn_validate_prepare_dims(const char* who, u32 D, u32 Dv);
// bsmr_softmax's rule: scale finite and > 0, and c = scale log2(e), rounded once from double,
// finite; else BSMR_ERR_INVALID with the message set
int attn_validate_scale(const char* who, float scale, float* c);
inline bool attn_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// lanes per lane group: max(D, Dv) sizeof(T) / 16 rounded up to a power of two, at least 4
inline u32 attn_lanes(u32 rowBytes) {
    u32 lanes = 4;
    while (lanes * 16u < rowBytes) lanes <<= 1;
    return lanes;
}
// the forward's segment chunk (ATTN_CHUNK of attention.hip)
u32 attn_forward_chunk();
// spmm_lists at side 1 over the plan's CSR in the plan's reordered row order, `chunk` entries per
// segment; layout_mu held. Synchronous on the plan's stream. `who` names the caller in errors
int attn_row_lists(const Plan& p, u32 chunk, const char* who, SpmmLists& L);

}  // namespace bsmr
