// row_elems.hpp — 16 bytes of a dense operand row as fp32 values, per operand dtype: what a lane
// of the gathering kernels (spmm.hip, attention.hip) unpacks after a 16-byte load.
#pragma once

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace bsmr {

// 16 bytes of a row as EPL fp32 values
template <int DT>
struct Elem;
template <>
struct Elem<BSMR_F32> {
    static constexpr int EPL = 4;
    static __device__ __forceinline__ void unpack(const uint4& q, float* x) {
        x[0] = __uint_as_float(q.x);
        x[1] = __uint_as_float(q.y);
        x[2] = __uint_as_float(q.z);
        x[3] = __uint_as_float(q.w);
    }
};
template <>
struct Elem<BSMR_BF16> {
    static constexpr int EPL = 8;
    static __device__ __forceinline__ void unpack(const uint4& q, float* x) {
        const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = __uint_as_float(w[i] << 16);
            x[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
        }
    }
};
template <>
struct Elem<BSMR_F16> {
    static constexpr int EPL = 8;
    static __device__ __forceinline__ void unpack(const uint4& q, float* x) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const h2 h = __builtin_bit_cast(h2, w[i]);
            x[2 * i] = static_cast<float>(h.x);
            x[2 * i + 1] = static_cast<float>(h.y);
        }
    }
};

}  // namespace bsmr
