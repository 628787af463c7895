// attention_common.hpp — what the fused attention forward (attention.hip) and backward
// (attention_bwd.hip) share on the host: the argument rules and the rows' segment lists (one copy,
// defined in attention.hip, so that the two entry points cannot drift apart). Also the operand
// record that the backward's kernels and launches are written with.
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
// one operand of a heads call against the layout rules (attention_layout.hpp, the only place they
// are written); else BSMR_ERR_INVALID with the message set: "<who>: <name>: <rule>"
int attn_check_operand(const char* who, const char* name, const bsmr_attention_operand* op, u32 batches, u32 heads,
                       u32 rows, u32 width, u32 esz, bool is_output);
// a b c saturating at the largest size_t: a scratch size that does not fit is never "ready" and
// never allocated
inline size_t attn_sat_mul(size_t a, size_t b, size_t c = 1) {
    size_t ab, abc;
    if (__builtin_mul_overflow(a, b, &ab) || __builtin_mul_overflow(ab, c, &abc)) return static_cast<size_t>(-1);
    return abc;
}
// slices = batches x heads of a prepare / prepared call: 1 .. the product of the two limits
int attn_check_slices(const char* who, u32 slices);
// one strided operand as the kernels take it: strides in bytes; a dimension of extent 1 is never
// stepped over, so its stride is dropped; a null operand (an output not asked for) is all zeros
struct AttnOpBytes {
    char* ptr;
    u64 batch, head;
    u32 row;
};
inline AttnOpBytes attn_op_bytes(const bsmr_attention_operand* op, u32 batches, u32 heads, u32 rows, u32 esz) {
    AttnOpBytes o{};
    if (!op) return o;
    o.ptr = static_cast<char*>(op->ptr);
    o.batch = batches > 1 ? op->batch * esz : 0;
    o.head = heads > 1 ? op->head * esz : 0;
    o.row = rows > 1 ? static_cast<u32>(op->row * esz) : 0;
    return o;
}
// the operand's base in slice (bat, head): wave-uniform, 64-bit, scalar registers
__device__ __forceinline__ char* attn_slice_base(const AttnOpBytes& op, u32 bat, u32 head) {
    return op.ptr + bat * op.batch + head * op.head;
}
// the forward's segment chunk (ATTN_CHUNK of attention.hip)
u32 attn_forward_chunk();
// spmm_lists at side 1 over the plan's CSR in the plan's reordered row order, `chunk` entries per
// segment; layout_mu held. Synchronous on the plan's stream. `who` names the caller in errors
int attn_row_lists(const Plan& p, u32 chunk, const char* who, SpmmLists& L);

}  // namespace bsmr
