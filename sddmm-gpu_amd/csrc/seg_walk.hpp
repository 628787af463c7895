// seg_walk.hpp — the loop at the centre of the gathering kernels as a function: one wave per
// segment of a gather list, the wave's 64 / L lane groups taking consecutive entries in the same
// instruction. k_attention_bwd_rows walks its segments with it; k_spmm, both phases of
// k_attention and k_attention_bwd_cols keep hand-written copies of the same loop, each because it
// measured slower on the walker. The summation order that the *_float64
// tests pin bit for bit is a property of this loop. The walker itself is plain C++
// (tests/seg_walk_main.cpp runs it on the host, lane by lane); shuffles, loads and arithmetic
// belong to the functors a kernel passes in. Below it, the lane-group geometry's users share a few
// small device helpers.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define BSMR_WALK_FN __host__ __device__ __forceinline__
#else
#define BSMR_WALK_FN inline
#endif

namespace bsmr {

using u32 = uint32_t;

// The lane groups of a wave: L lanes (a power of two <= 64) cover a row with 16-byte loads, the
// G = 64 / L groups take G consecutive entries per instruction; this lane is lane l of group g
struct LaneGroups {
    u32 L, G, g, l;
    BSMR_WALK_FN LaneGroups(u32 lanes, u32 lane) : L(lanes), G(64u / lanes), g(lane / lanes), l(lane % lanes) {}
};

// Walks a segment of `count` entries in batches of 64, one record per lane:
//   load(b0)                      the lane's record of entry b0 + lane (whatever the kernel keeps per
//                                 entry: an index, or an index with its values);
//   fetch(batch, idx, valid, e)   shuffles entry idx's record out of the batch and issues its gathers;
//   use(e, b0 + idx, valid)       consumes one entry.
// `first` is batch 0, already loaded (a caller that walks a segment twice can load it once). The
// next batch's load is issued before the current batch's first fetch, so that it lands under the
// gathers. A step is U entries per lane group: its U fetches, then its U uses in entry order (U
// rows in flight per lane). Group g takes entries g, g + G, ... of a batch; the steps left over
// after the last whole U go one at a time, and the last may be partly filled: every lane still
// makes both calls (an idle lane may hold another's record, and a butterfly needs all lanes), with
// valid = false, and the functors predicate their loads and sums on it.
template <u32 U, class Ent, class Batch, class Load, class Fetch, class Use>
BSMR_WALK_FN void seg_walk(u32 count, u32 G, u32 g, Batch first, Load load, Fetch fetch, Use use) {
    Batch cur = first;
    for (u32 b0 = 0; b0 < count; b0 += 64u) {
        Batch next = cur;
        if (b0 + 64u < count) next = load(b0 + 64u);
        const u32 nb = count - b0 < 64u ? count - b0 : 64u;
        const u32 full = nb / G;  // steps in which every lane group has an entry
        u32 j = 0;
        for (; j + U <= full; j += U) {
            Ent e[U];
#pragma unroll
            for (u32 u = 0; u < U; ++u) fetch(cur, (j + u) * G + g, true, e[u]);
#pragma unroll
            for (u32 u = 0; u < U; ++u) use(e[u], b0 + (j + u) * G + g, true);
        }
        for (; j * G < nb; ++j) {  // the remaining steps; the last may be partly filled
            const u32 idx = j * G + g;
            const bool valid = idx < nb;
            Ent e;
            fetch(cur, idx, valid, e);
            use(e, b0 + idx, valid);
        }
        cur = next;
    }
}

#ifdef __HIPCC__

// v_exp_f32: 2^x to 1 ulp, 0 for -inf (and for results under 2^-126)
__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }

// a lane group's dot product: the lane's FMA chain in element order from 0, then the xor butterfly
// from L / 2 down to 1 (every lane of the group ends with the sum)
template <int EPL>
__device__ __forceinline__ float group_dot(const float* a, const float* b, u32 L) {
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < EPL; ++i) d = __builtin_fmaf(a[i], b[i], d);
    for (u32 off = L >> 1; off >= 1u; off >>= 1) d += __shfl_xor(d, static_cast<int>(off));
    return d;
}

// EPL fp32 values of the row at `row`, from element l EPL on
template <int EPL>
__device__ __forceinline__ void load_f32(const char* row, u32 l, float* x) {
    const float4* p = reinterpret_cast<const float4*>(row) + static_cast<size_t>(l) * (EPL / 4);
#pragma unroll
    for (int i = 0; i < EPL; i += 4) {
        const float4 v = p[i / 4];
        x[i] = v.x;
        x[i + 1] = v.y;
        x[i + 2] = v.z;
        x[i + 3] = v.w;
    }
}

template <int EPL>
__device__ __forceinline__ void store_f32(float* o, const float* x) {
#pragma unroll
    for (int i = 0; i < EPL; i += 4) *reinterpret_cast<float4*>(o + i) = make_float4(x[i], x[i + 1], x[i + 2], x[i + 3]);
}

#endif  // __HIPCC__

}  // namespace bsmr
