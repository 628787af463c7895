// panel_mfma.hpp — what the panel kernels share on the device (attention_panels.hip, the attention
// forward; attention_panels_kv8.hip and attention_panels_kv4.hip, its e4m3 and MXFP4 K / V forms;
// attention_bwd_panels.hip, the backward's rows and columns kernels; spmm_panels.hip, the SpMM of the SDDMM gradients), and the one place
// that states their lane mapping, k-slot order and stage layout.
//
// Lane mapping. A wave takes an item: up to PANEL_ITEM_STEPS steps of 32 sources (columns; union
// rows on a columns side) for a panel's 16 destinations. Lane l of the wave is (r, g) = (l & 15,
// l >> 4) everywhere, and for v_mfma_f32_16x16x32_{f16,bf16}
//   A operand  lane (i, g) holds A[i][8 g, +8)        (16 x 32)
//   B operand  lane (n, g) holds B[8 g, +8)[n]        (32 x 16)
//   result     lane (n, g) holds C[4 g + j][n], j = 0 .. 3
// Every product is transposed so that the destination is on the N side: lane (r, g) keeps
// everything of destination r and nothing is shuffled between a first product and a second.
//
// k-slot order. A first product over the step's two 16-source tiles leaves lane (r, g) with the
// values of destination r at step slots 4 g + j (tile 0) and 16 + 4 g + j (tile 1), j = 0 .. 3.
// Those eight, packed in that order (pack8), are the lane's B operand of the second product:
// k-slot 8 g + j is step slot panel_slot(g, j). The A operand of the second product (staged_pair,
// staged_quad), the mask selects and the SpMM's weights follow the same function.
//
// Stage layout. The step's 32 source rows are staged in the wave's own LDS by 16-byte loads and
// stores (chunk x = 64 u + lane is 16 bytes of row x / CPR, CPR chunks per row, so every row is
// fetched once per step), rows staged_row_bytes(width) = 2 width + 16 bytes apart. staged_pair's
// lane (i, g) reads the 32-bit word of elements (32 n + 2 i, + 1) of its eight rows: word index
// (4 g + j)(width / 2 + 4) + 16 n + i. width / 2 is a multiple of 16, so 4 g (width / 2 + 4) is
// 16 g (mod 64) and the index is 16 g + i + const (mod 64): one instruction's 64 reads fall on 64
// different banks. (A padding of 4 or 12 words mod 16 does that; 16 bytes also keeps the rows
// aligned for the 16-byte stores.) A wave orders its own stores and loads with wave_lds_sync; no
// workgroup barrier is needed.
//
// Sharing rule: a step stands here only if every kernel that uses it
// compiles to the instructions it had with the step written in place. The item prologue, the stage
// loop, the online-softmax step, the row sum of l and a store_acc with a per-element operation did
// not, as functions, in any parameter form, and stay written in each kernel.
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

// step slot of a lane's j-th value, j = 0 .. 7 (the k-slot order)
__device__ __forceinline__ constexpr u32 panel_slot(u32 g, int j) { return j < 4 ? 4u * g + j : 16u + 4u * g + (j - 4); }

// a lane's eight values of a step, in k-slot order, as the B operand of the second product
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

// An e8m0 scale byte s as the float the fp4 convert takes: bits s << 23, that is 2^(s - 127) for
// s = 1 .. 254, +inf for 0xFF (the convert reads the exponent field alone and makes the block NaN)
// and +0 for 0 (read as 2^-127)
__device__ __forceinline__ float mx_scale(u32 s) { return __builtin_bit_cast(float, s << 23); }

// Byte SEL of w, two e2m1 nibbles, times `scale` (mx_scale) widened to the operand type by gfx950's
// packed convert: the low nibble lands in the low half. Exact where nibble x scale is a normal
// number of the type (fp16: block exponents -13 .. 13 for every nibble; bf16: -125 .. 125)
template <int DT, int SEL>
__device__ __forceinline__ u32 widen2_fp4(u32 w, float scale) {
    if constexpr (DT == BSMR_F16)
        return __builtin_bit_cast(u32, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, SEL));
    else
        return __builtin_bit_cast(u32, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, SEL));
}

// a word of eight e2m1 nibbles of one block as an operand of mfma32, in element order
template <int DT>
__device__ __forceinline__ uint4 widen8_fp4(u32 w, float scale) {
    return make_uint4(widen2_fp4<DT, 0>(w, scale), widen2_fp4<DT, 1>(w, scale), widen2_fp4<DT, 2>(w, scale),
                      widen2_fp4<DT, 3>(w, scale));
}

__device__ __forceinline__ uint4 load16(const char* p) { return *reinterpret_cast<const uint4*>(p); }

// a wave synchronises with itself only: its LDS stores before, its LDS loads after
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bytes between the staged rows of a tile of `width` 16-bit elements (the stage layout above)
__host__ __device__ constexpr u32 staged_row_bytes(u32 width) { return 2u * width + 16u; }

// lane (r, g)'s operand registers of a 16-bit row for the whole item: elements [32 s + 8 g, +8) of
// every k-step s; zeros when the row is not live
template <int KS>
__device__ __forceinline__ void panel_row_operand(uint4 (&q)[KS], const char* rowp, bool live, u32 g) {
#pragma unroll
    for (int s = 0; s < KS; ++s) q[s] = live ? load16(rowp + (32u * s + 8u * g) * 2u) : make_uint4(0, 0, 0, 0);
}

// The A operands of two MFMAs of the second product from a step's 32 staged rows (ROW bytes
// apart): lane (i, g) reads the 32-bit word of elements (32 n + 2 i, 32 n + 2 i + 1) of its eight
// rows (k-slot order) and splits it with two byte permutes per row pair: `even` is element
// 32 n + 2 i of the eight rows, `odd` element 32 n + 2 i + 1. With the lane's packed eight values
// as B, lane (r, g) then accumulates elements 32 n + 8 g + 2 j (even) and + 2 j + 1 (odd) of r
template <u32 ROW>
__device__ __forceinline__ void staged_pair(const char* tile, u32 n, u32 i, u32 g, uint4& even, uint4& odd) {
    u32 w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = *reinterpret_cast<const u32*>(tile + panel_slot(g, j) * ROW + (32u * n + 2u * i) * 2u);
    even.x = __builtin_amdgcn_perm(w[1], w[0], 0x05040100u), odd.x = __builtin_amdgcn_perm(w[1], w[0], 0x07060302u);
    even.y = __builtin_amdgcn_perm(w[3], w[2], 0x05040100u), odd.y = __builtin_amdgcn_perm(w[3], w[2], 0x07060302u);
    even.z = __builtin_amdgcn_perm(w[5], w[4], 0x05040100u), odd.z = __builtin_amdgcn_perm(w[5], w[4], 0x07060302u);
    even.w = __builtin_amdgcn_perm(w[7], w[6], 0x05040100u), odd.w = __builtin_amdgcn_perm(w[7], w[6], 0x07060302u);
}

// acc[2 n][j] and acc[2 n + 1][j] (staged_pair's even and odd) are elements 32 n + 8 g + 2 j and
// + 2 j + 1 of the lane's row: o points at element 8 g
template <int NP>
__device__ __forceinline__ void store_acc(float* o, const f32x4* acc) {
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        const f32x4 e = acc[2 * n], d = acc[2 * n + 1];
        *reinterpret_cast<float4*>(o + 32 * n) = make_float4(e[0], d[0], e[1], d[1]);
        *reinterpret_cast<float4*>(o + 32 * n + 4) = make_float4(e[2], d[2], e[3], d[3]);
    }
}

}  // namespace bsmr
