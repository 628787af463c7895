// softmax.hip — row softmax over the plan's pattern for gfx950 (bsmr_softmax, bsmr_softmax_backward):
// the step between bsmr_sddmm's scores and the aggregation bsmr_spmm.
//
//   forward   d_e = (P_e - max_i P) scale, t_e = exp(d_e), W_e = t_e / sum_i t
//   backward  dP_e = scale W_e (G_e - sum_i W G)
//
// A CSR row is contiguous in P, so the item list (softmax_schedule.cpp) names rows only. Packed
// runs and wave rows share one launch at 16 waves per workgroup, one item per wave; block rows
// take a second launch, one workgroup each. A wave or workgroup of T threads holds a pass of 16 T
// entries in registers: entry k of the pass sits in thread (k / 4) % T, register 4 (k / 4 / T) +
// k % 4, loaded 16 bytes at a time when the row starts on a 16-byte boundary and by 4-byte loads
// otherwise, into the same registers. A thread reduces its registers in index order, a lane group or
// wave reduces by the xor butterfly from the widest offset down, a workgroup adds its 16 wave
// partials in wave order through LDS, passes are combined in pass order: the order is a function
// of the row's length alone. fp32 throughout; no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "plan.hpp"
#include "softmax_schedule.hpp"

namespace bsmr {
namespace {

constexpr u32 SM_WAVES = 16;  // waves (items) per workgroup of the packed / wave launch
constexpr int SM_REGS = static_cast<int>(SOFTMAX_REGS);
static_assert(SOFTMAX_REGS % 4 == 0 && SOFTMAX_BLOCK_WAVES == 16, "register quads; 1024-thread block rows");

struct SoftmaxArgs {
    const SoftmaxItem* items;
    const u32* rowptr;
    const float* in0;  // P (forward), W (backward)
    const float* in1;  // G (backward)
    float* out;        // W (forward), dP (backward)
    u32 nItems;
    float c;           // forward: scale log2(e), rounded once from double; backward: scale
};

// v_exp_f32: 2^x to 1 ulp, 0 for -inf (and for results under 2^-126)
__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }

struct OpMax {
    static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); }
};
struct OpSum {
    static __device__ __forceinline__ float f(float a, float b) { return a + b; }
};

// the value of all T = 64 WAVES threads reduced: butterfly inside a wave, then the wave partials
// in wave order (every thread reads the same partials, so every thread holds the same result)
template <int WAVES, class Op>
__device__ __forceinline__ float team_reduce(float v, float* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = Op::f(v, __shfl_xor(v, off));
    if constexpr (WAVES > 1) {
        __syncthreads();  // the partials of the reduction before this one have been read
        if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v = Op::f(v, lds[w]);
    }
    return v;
}

// n <= 16 T entries at p into thread t's registers (header comment); entries past n hold `fill`
template <u32 T>
__device__ __forceinline__ void load_tile(const float* p, u32 n, u32 t, float fill, float (&x)[SM_REGS]) {
    const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
#pragma unroll
    for (int q = 0; q < SM_REGS / 4; ++q) {
        const u32 k = (q * T + t) * 4u;
        if (aligned && k + 4u <= n) {
            const float4 v = *reinterpret_cast<const float4*>(p + k);
            x[4 * q] = v.x;
            x[4 * q + 1] = v.y;
            x[4 * q + 2] = v.z;
            x[4 * q + 3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[4 * q + i] = k + i < n ? p[k + i] : fill;
        }
    }
}

template <u32 T>
__device__ __forceinline__ void store_tile(float* p, u32 n, u32 t, const float (&x)[SM_REGS]) {
    const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
#pragma unroll
    for (int q = 0; q < SM_REGS / 4; ++q) {
        const u32 k = (q * T + t) * 4u;
        if (aligned && k + 4u <= n) {
            *reinterpret_cast<float4*>(p + k) = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k + i < n) p[k + i] = x[4 * q + i];
        }
    }
}

// the maximum a row's entries are shifted by: 0 for a row whose entries are all -inf (they then
// keep d = -inf, t = 0, instead of -inf - -inf = NaN)
__device__ __forceinline__ float shift_of(float m) { return m == -INFINITY ? 0.f : m; }
// 1 / sum; a sum of 0 is the fully masked row (a live maximum contributes exp(0) = 1): weights 0
__device__ __forceinline__ float inverse_of(float s) { return s == 0.f ? 0.f : 1.0f / s; }

// one row of `len` entries by 64 WAVES threads, thread t. A row of one pass is read once; a longer
// one keeps a running (max, sum) over its passes, rescaled when the maximum grows, and reads P a
// second time for the weights. In place (out == in0): a thread writes only what it read, after the
// last reduction of the first sweep.
template <int WAVES>
__device__ __forceinline__ void row_forward(const SoftmaxArgs& a, u32 first, u32 len, u32 t, float* lds) {
    constexpr u32 T = 64u * WAVES, PASS = T * SOFTMAX_REGS;
    const float* p = a.in0 + first;
    float* o = a.out + first;
    const u32 passes = (len + PASS - 1) / PASS;
    float x[SM_REGS];
    float m = -INFINITY, shift = 0.f, s = 0.f;
    for (u32 ps = 0; ps < passes; ++ps) {
        const u32 b = ps * PASS;
        load_tile<T>(p + b, min(PASS, len - b), t, -INFINITY, x);
        float pm = x[0];
#pragma unroll
        for (int j = 1; j < SM_REGS; ++j) pm = fmaxf(pm, x[j]);
        const float mn = fmaxf(m, team_reduce<WAVES, OpMax>(pm, lds));
        shift = shift_of(mn);
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < SM_REGS; ++j) {
            x[j] = exp2_hw((x[j] - shift) * a.c);
            acc += x[j];
        }
        acc = team_reduce<WAVES, OpSum>(acc, lds);
        s = s * exp2_hw((m - shift) * a.c) + acc;  // the first pass: 0 * 2^-inf + acc
        m = mn;
    }
    const float inv = inverse_of(s);
    if (passes == 1) {
#pragma unroll
        for (int j = 0; j < SM_REGS; ++j) x[j] *= inv;
        store_tile<T>(o, len, t, x);
        return;
    }
    for (u32 ps = 0; ps < passes; ++ps) {
        const u32 b = ps * PASS, n = min(PASS, len - b);
        load_tile<T>(p + b, n, t, -INFINITY, x);
#pragma unroll
        for (int j = 0; j < SM_REGS; ++j) x[j] = exp2_hw((x[j] - shift) * a.c) * inv;
        store_tile<T>(o + b, n, t, x);
    }
}

template <int WAVES>
__device__ __forceinline__ void row_backward(const SoftmaxArgs& a, u32 first, u32 len, u32 t, float* lds) {
    constexpr u32 T = 64u * WAVES, PASS = T * SOFTMAX_REGS;
    const float* w = a.in0 + first;
    const float* g = a.in1 + first;
    float* o = a.out + first;
    const u32 passes = (len + PASS - 1) / PASS;
    float xw[SM_REGS], xg[SM_REGS];
    float r = 0.f;
    for (u32 ps = 0; ps < passes; ++ps) {
        const u32 b = ps * PASS, n = min(PASS, len - b);
        load_tile<T>(w + b, n, t, 0.f, xw);
        load_tile<T>(g + b, n, t, 0.f, xg);
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < SM_REGS; ++j) acc = __builtin_fmaf(xw[j], xg[j], acc);
        r += team_reduce<WAVES, OpSum>(acc, lds);
    }
    for (u32 ps = 0; ps < passes; ++ps) {
        const u32 b = ps * PASS, n = min(PASS, len - b);
        if (passes > 1) {
            load_tile<T>(w + b, n, t, 0.f, xw);
            load_tile<T>(g + b, n, t, 0.f, xg);
        }
#pragma unroll
        for (int j = 0; j < SM_REGS; ++j) xg[j] = a.c * (xw[j] * (xg[j] - r));
        store_tile<T>(o + b, n, t, xg);
    }
}

// a packed run: lane group g (L lanes) takes row it.row + g, one entry per lane; the butterfly
// stays inside the group. Groups past the run and groups of empty rows idle (they write nothing)
template <bool BWD, u32 L>
__device__ __forceinline__ void packed_run(const SoftmaxArgs& a, const SoftmaxItem& it, u32 lane) {
    const u32 g = lane / L, l = lane & (L - 1u);
    u32 e0 = 0, n = 0;
    if (g < it.count) {
        e0 = a.rowptr[it.row + g];
        n = a.rowptr[it.row + g + 1u] - e0;
    }
    const bool live = l < n;
    const size_t e = static_cast<size_t>(e0) + l;
    if constexpr (!BWD) {
        const float x = live ? a.in0[e] : -INFINITY;
        float m = x;
#pragma unroll
        for (u32 off = L >> 1; off >= 1u; off >>= 1) m = fmaxf(m, __shfl_xor(m, static_cast<int>(off)));
        const float tv = exp2_hw((x - shift_of(m)) * a.c);
        float s = tv;
#pragma unroll
        for (u32 off = L >> 1; off >= 1u; off >>= 1) s += __shfl_xor(s, static_cast<int>(off));
        if (live) a.out[e] = tv * inverse_of(s);
    } else {
        const float w = live ? a.in0[e] : 0.f;
        const float gv = live ? a.in1[e] : 0.f;
        float r = w * gv;
#pragma unroll
        for (u32 off = L >> 1; off >= 1u; off >>= 1) r += __shfl_xor(r, static_cast<int>(off));
        if (live) a.out[e] = a.c * (w * (gv - r));
    }
}

// packed runs and wave rows: one item per wave, its descriptor wave-uniform (scalar loads). At most
// 64 VGPRs: a workgroup is 4 waves per SIMD, so 8 waves per SIMD is two resident workgroups and 7
// would be one (measured on the cop20k-like pattern, DESIGN.md §12: forward / backward 19.0 /
// 19.6 us at 66 / 67 VGPRs, 12.7 / 13.0 us at 64)
template <bool BWD>
__global__ __launch_bounds__(SM_WAVES * 64) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_softmax_rows(const SoftmaxArgs a) {
    const u32 lane = threadIdx.x & 63u;
    const u32 id = blockIdx.x * SM_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (id >= a.nItems) return;
    const SoftmaxItem it = a.items[id];
    if (it.kind == SOFTMAX_WAVE) {
        if constexpr (BWD) row_backward<1>(a, it.first, it.count, lane, nullptr);
        else row_forward<1>(a, it.first, it.count, lane, nullptr);
    } else {
        switch (it.kind) {  // the lane-group width, a compile-time constant in each butterfly
            case 1: packed_run<BWD, 1>(a, it, lane); break;
            case 2: packed_run<BWD, 2>(a, it, lane); break;
            case 4: packed_run<BWD, 4>(a, it, lane); break;
            case 8: packed_run<BWD, 8>(a, it, lane); break;
            case 16: packed_run<BWD, 16>(a, it, lane); break;
            case 32: packed_run<BWD, 32>(a, it, lane); break;
            default: packed_run<BWD, 64>(a, it, lane); break;
        }
    }
}

// block rows: one row per workgroup of 16 waves
template <bool BWD>
__global__ __launch_bounds__(SOFTMAX_BLOCK_WAVES * 64) void k_softmax_block(const SoftmaxArgs a) {
    __shared__ float lds[SOFTMAX_BLOCK_WAVES];
    const SoftmaxItem it = a.items[blockIdx.x];
    if constexpr (BWD) row_backward<SOFTMAX_BLOCK_WAVES>(a, it.first, it.count, threadIdx.x, lds);
    else row_forward<SOFTMAX_BLOCK_WAVES>(a, it.first, it.count, threadIdx.x, lds);
}

// build the item list and upload it, packed runs and wave rows apart from block rows (each in
// ascending row order); layout_mu held. Synchronous on the plan's stream.
int build_softmax(const Plan& p) {
    Plan::SoftmaxList& S = p.softmax;
    if (S.built) return BSMR_OK;
    const hipStream_t s = p.stream;
    std::vector<u32> hrp;
    BSMR_CHECK(p.rowptr.download(hrp, s));
    SoftmaxItems L;
    std::string err;
    if (hrp.size() != static_cast<size_t>(p.M) + 1 || softmax_items(p.M, hrp.data(), L, err)) {
        set_error("bsmr_plan_prepare_softmax: " + (err.empty() ? std::string("the plan holds no rowptr") : err));
        return BSMR_ERR_INVALID;
    }
    std::vector<SoftmaxItem> rows, blocks;
    for (const SoftmaxItem& it : L.items) (it.kind == SOFTMAX_BLOCK ? blocks : rows).push_back(it);
    BSMR_CHECK(S.rows.upload(rows.data(), rows.size(), s));
    BSMR_CHECK(S.blocks.upload(blocks.data(), blocks.size(), s));
    BSMR_HIP(hipStreamSynchronize(s));
    S.nRows = static_cast<u32>(rows.size());
    S.nBlocks = static_cast<u32>(blocks.size());
    S.packedRuns = L.packedRuns;
    S.waveRows = L.waveRows;
    S.maxRow = L.maxRow;
    S.built = true;
    return BSMR_OK;
}

int launch_softmax(const bsmr_plan* plan, bool bwd, const float* in0, const float* in1, float scale, float* out,
                   void* stream) {
    const char* who = bwd ? "bsmr_softmax_backward" : "bsmr_softmax";
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    if (!in0 || !out || (bwd && !in1)) {
        set_error(std::string(who) + ": null device pointer");
        return BSMR_ERR_INVALID;
    }
    // the forward's exponent factor, rounded once; both directions take the same scales
    const float c2 = static_cast<float>(static_cast<double>(scale) * 1.4426950408889634);
    const float c = bwd ? scale : c2;
    if (!(scale > 0.f) || !std::isfinite(scale) || !std::isfinite(c2)) {
        set_error(std::string(who) + ": scale must be finite and > 0 (and scale * log2(e) finite)");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    SoftmaxArgs a{};
    const SoftmaxItem* blocks = nullptr;
    u32 nBlocks = 0;
    {
        std::lock_guard<std::mutex> g(p.layout_mu);
        if (!p.softmax.built) {
            const LaunchSite at{s, who, "bsmr_plan_prepare_softmax", 0, BSMR_F32};
            const int st = lazy_build_guard(at);
            if (st == BSMR_ERR_NOT_PREPARED)  // (the guard's own message names a (K, dtype) layout)
                set_error(std::string(who) + ": stream is capturing and the softmax item list is not built; "
                                             "call bsmr_plan_prepare_softmax first");
            BSMR_CHECK(st);
            BSMR_CHECK(build_softmax(p));
        }
        a.items = p.softmax.rows.data();
        a.nItems = p.softmax.nRows;
        blocks = p.softmax.blocks.data();
        nBlocks = p.softmax.nBlocks;
    }
    a.rowptr = p.rowptr.data();
    a.in0 = in0;
    a.in1 = in1;
    a.out = out;
    a.c = c;
    if (a.nItems) {
        const u32 grid = (a.nItems + SM_WAVES - 1) / SM_WAVES;
        hipLaunchKernelGGL(bwd ? k_softmax_rows<true> : k_softmax_rows<false>, dim3(grid), dim3(SM_WAVES * 64), 0, s,
                           a);
        BSMR_HIP(hipGetLastError());
    }
    if (nBlocks) {
        a.items = blocks;
        a.nItems = nBlocks;
        hipLaunchKernelGGL(bwd ? k_softmax_block<true> : k_softmax_block<false>, dim3(nBlocks),
                           dim3(SOFTMAX_BLOCK_WAVES * 64), 0, s, a);
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

}  // namespace
}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_softmax(const bsmr_plan* plan, const float* dP, float scale, float* dW, void* stream) {
    return launch_softmax(plan, false, dP, nullptr, scale, dW, stream);
}

extern "C" int bsmr_softmax_backward(const bsmr_plan* plan, const float* dW, const float* dG, float scale,
                                     float* dGP, void* stream) {
    return launch_softmax(plan, true, dW, dG, scale, dGP, stream);
}

extern "C" int bsmr_plan_prepare_softmax(const bsmr_plan* plan) {
    if (!plan) {
        set_error("bsmr_plan_prepare_softmax: null plan");
        return BSMR_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_softmax(plan->p);
}

extern "C" int bsmr_plan_softmax_prepared(const bsmr_plan* plan) {
    if (!plan) {
        set_error("bsmr_plan_softmax_prepared: null plan");
        return 0;
    }
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return plan->p.softmax.built ? 1 : 0;
}

extern "C" int bsmr_plan_softmax_stats(const bsmr_plan* plan, bsmr_softmax_stats* out) {
    if (!plan || !out) {
        set_error("bsmr_plan_softmax_stats: null argument");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    const Plan::SoftmaxList& S = p.softmax;
    *out = bsmr_softmax_stats{};
    out->wave_max = SOFTMAX_WAVE_MAX;
    out->block_pass = SOFTMAX_BLOCK_PASS;
    if (S.built) {
        out->items = S.nRows + S.nBlocks;
        out->packed_runs = S.packedRuns;
        out->wave_rows = S.waveRows;
        out->block_rows = S.nBlocks;
        out->max_row = S.maxRow;
    }
    return BSMR_OK;
}
