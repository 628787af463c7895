// panel_mfma.hpp — what the panel kernels of the fused sparse attention share on the device
// (attention_panels.hip, the forward; attention_bwd_panels.hip, the backward): the 16 x 16 x 32
// matrix instruction on fp16 / bf16 operands, the rounding pack, the exact widening of e4m3 bytes
// (attention_panels_kv8.hip), the wave's own LDS ordering and the transposing read of a staged tile. Lane l of a wave is (r, g) = (l & 15, l >> 4) everywhere:
//   A operand  lane (i, g) holds A[i][8 g, +8)        (16 x 32)
//   B operand  lane (n, g) holds B[8 g, +8)[n]        (32 x 16)
//   result     lane (n, g) holds C[4 g + j][n], j = 0 .. 3
// so with the per-row (per-column) quantity on the N side, lane (r, g) keeps everything of r.
#pragma once

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace bsmr {

constexpr u32 PANEL_WAVES = 4;  // waves (items) per workgroup

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 b16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 b16x8 __attribute__((ext_vector_type(8)));

template <int DT>
__device__ __forceinline__ f32x4 mfma32(const uint4& a, const uint4& b, const f32x4 c) {
    if constexpr (DT == BSMR_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b16x8, a), __builtin_bit_cast(b16x8, b), c, 0, 0, 0);
}

// two fp32 values rounded to the operand type (nearest even), lo in the low half
template <int DT>
__device__ __forceinline__ u32 pack2(float lo, float hi) {
    if constexpr (DT == BSMR_F16) {
        const h16x2 h = {static_cast<_Float16>(lo), static_cast<_Float16>(hi)};
        return __builtin_bit_cast(u32, h);
    } else {
        const b16x2 h = {static_cast<__bf16>(lo), static_cast<__bf16>(hi)};
        return __builtin_bit_cast(u32, h);
    }
}

// a lane's eight values of a step (step columns 4 g + j for j < 4, 16 + 4 g + j - 4 else) as the B
// operand of the second product: k-slot 8 g + j
template <int DT>
__device__ __forceinline__ uint4 pack8(const float* t) {
    return make_uint4(pack2<DT>(t[0], t[1]), pack2<DT>(t[2], t[3]), pack2<DT>(t[4], t[5]), pack2<DT>(t[6], t[7]));
}

// Two OCP e4m3 bytes (the low or the high half of w) widened to the operand type by gfx950's packed
// convert with scale 1: exact, since an e4m3 value (3 mantissa bits, 2^-9 .. 2^8) is a normal
// number of fp16 and of bf16; a NaN byte (0x7F, 0xFF) stays a NaN. The lower byte lands in the low half
template <int DT, bool HI>
__device__ __forceinline__ u32 widen2(u32 w) {
    if constexpr (DT == BSMR_F16)
        return __builtin_bit_cast(u32, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
    else
        return __builtin_bit_cast(u32, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
}

// eight consecutive e4m3 bytes (two words) as an operand of mfma32, in byte order
template <int DT>
__device__ __forceinline__ uint4 widen8(u32 lo, u32 hi) {
    return make_uint4(widen2<DT, false>(lo), widen2<DT, true>(lo), widen2<DT, false>(hi), widen2<DT, true>(hi));
}

__device__ __forceinline__ uint4 load16(const char* p) { return *reinterpret_cast<const uint4*>(p); }

// a wave synchronises with itself only: its LDS stores before, its LDS loads after
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bytes between the staged rows of a tile of `width` 16-bit elements: 2 width + 16, so that the
// 64 word reads of staged_pair fall on 64 different banks
__host__ __device__ constexpr u32 staged_row_bytes(u32 width) { return 2u * width + 16u; }

// The A operands of two MFMAs of the second product from a step's 32 staged rows (ROW bytes
// apart): lane (i, g) reads the 32-bit word of elements (32 n + 2 i, 32 n + 2 i + 1) of its eight
// rows (k-slot order) and splits it with two byte permutes per row pair: `even` is element
// 32 n + 2 i of the eight rows, `odd` element 32 n + 2 i + 1. With the lane's packed eight values
// as B, lane (r, g) then accumulates elements 32 n + 8 g + 2 j (even) and + 2 j + 1 (odd) of r
template <u32 ROW>
__device__ __forceinline__ void staged_pair(const char* tile, u32 n, u32 i, u32 g, uint4& even, uint4& odd) {
    u32 w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const u32 cc = (j < 4 ? 4u * g + j : 16u + 4u * g + (j - 4));
        w[j] = *reinterpret_cast<const u32*>(tile + cc * ROW + (32u * n + 2u * i) * 2u);
    }
    even.x = __builtin_amdgcn_perm(w[1], w[0], 0x05040100u), odd.x = __builtin_amdgcn_perm(w[1], w[0], 0x07060302u);
    even.y = __builtin_amdgcn_perm(w[3], w[2], 0x05040100u), odd.y = __builtin_amdgcn_perm(w[3], w[2], 0x07060302u);
    even.z = __builtin_amdgcn_perm(w[5], w[4], 0x05040100u), odd.z = __builtin_amdgcn_perm(w[5], w[4], 0x07060302u);
    even.w = __builtin_amdgcn_perm(w[7], w[6], 0x05040100u), odd.w = __builtin_amdgcn_perm(w[7], w[6], 0x07060302u);
}

}  // namespace bsmr
