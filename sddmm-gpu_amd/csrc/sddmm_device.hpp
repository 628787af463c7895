// sddmm_device.hpp — the few device helpers the column-major kernels (sddmm.hip) and the row-block
// kernel (rb_kernel.hpp) share: 16-byte loads, DPP moves on 16-lane rows and the BSMR_DIAG & 32
// timeline. Included by sddmm.hip only; everything here is internal to that translation unit.
#pragma once

#include "common.hpp"

namespace bsmr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// debug timeline (BSMR_DIAG & 32 only): wave start / mid / end in s_memrealtime ticks (100 MHz)
// and the wave's XCC id << 32 | HW_ID register
__device__ __forceinline__ unsigned long long rtime(const void* on) {
    return on ? __builtin_amdgcn_s_memrealtime() : 0ull;
}
__device__ __forceinline__ void trace_wave(unsigned long long* tr, u32 slot, unsigned long long t0,
                                           unsigned long long tm, unsigned long long td = 0) {
    if (tr && __lane_id() == 0) {
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        const u32 xcc = __builtin_amdgcn_s_getreg(0xF814);  // HW_REG_XCC_ID, 32 bits
        tr[4ull * slot + 0] = t0;
        tr[4ull * slot + 1] = tm;
        tr[4ull * slot + 2] = t1;
        tr[4ull * slot + 3] = (static_cast<unsigned long long>(xcc) << 60) | (td ? td : tm);
    }
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// DPP helpers on 16-lane rows (VALU only, no LDS crossbar)
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v),
                                                                 CTRL, 0xF, 0xF, false));
}
// value of lane N of the row, in every lane of the row (row_newbcast, gfx90a+)
template <int N>
__device__ __forceinline__ u32 row_bcast(u32 v) {
    return static_cast<u32>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x150 + N, 0xF, 0xF,
                                                         false));
}

}  // namespace
}  // namespace bsmr
