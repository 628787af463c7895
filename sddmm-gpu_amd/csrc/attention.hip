// attention.hip — fused sparse attention forward for gfx950 (bsmr_attention):
//
//   O[i,:] = sum_e W_e V[j_e,:],  W = softmax over row i of scale dot(Q[i,:], K[j_e,:])
//
// in one launch (two with split rows), without the nnz-sized scores and weights of the chain
// bsmr_sddmm -> bsmr_softmax -> bsmr_spmm. One wave per segment of a row (spmm_lists at side 1,
// ATTN_CHUNK entries at most), 16 waves per workgroup. L = max(D, Dv) sizeof(T) / 16 lanes
// (rounded up to a power of two) cover a K row and a V row with 16-byte loads, and the 64 / L
// lane groups of the wave take consecutive entries of the segment in the same instruction.
//   phase 1: group g gathers the K rows of entries g, g + G, ...; a lane's partial dot product
//            (one FMA per element, in element order) is reduced inside the group by the xor
//            butterfly from the widest offset down; the segment's scores stay in LDS (1 KiB
//            per wave) and its maximum m is a wave butterfly;
//   phase 2: the same group takes t_e = 2^((p_e - m) c), c = scale log2(e) rounded once from
//            double, adds it to its l and takes one FMA per column into its accumulator, in
//            entry order; then the groups' (l, acc) are added in group order.
// Nothing is rescaled inside a segment. A row of one segment stores acc (1 / l) and m scale +
// ln l; a segment of a split row writes (m, l, acc) to plan-owned scratch and k_attention_reduce
// takes M = max m_s, scales each partial once by 2^((m_s - M) c) and adds l and acc in segment
// order. fp32 accumulation throughout; no atomics: the order is a function of the row's length,
// D, Dv and the dtype alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "attention_common.hpp"
#include "plan.hpp"
#include "row_elems.hpp"
#include "spmm_schedule.hpp"

namespace bsmr {
namespace {

// entries per segment; a macro so that an A/B build can override it (-DATTN_CHUNK=...).
// Measured at D = Dv = 64 fp32: C2 41.4 us at 128, 37.7 us at 256 (half the
// partials); C3 (no row over 31 entries) 128.7 / 128.6 us
#ifndef ATTN_CHUNK
#define ATTN_CHUNK 256
#endif
constexpr u32 ATTN_WAVES = 16;     // waves (segments) per workgroup, as k_spmm
static_assert(ATTN_CHUNK % 64 == 0 && ATTN_CHUNK >= 64 && ATTN_CHUNK <= 1024, "batches of 64; scores in LDS");

struct AttnArgs {
    const SpmmSeg* segs;
    const u32* colidx;
    const char* Q;      // M rows of kBytes
    const char* K;      // N rows of kBytes
    const char* V;      // N rows of vBytes
    float* O;           // M x Dv
    float* lse;         // M, or null
    float* pacc;        // partial slots x Dv
    float* pml;         // partial slots x (m, l)
    u32 nSegs, Dv, kBytes, vBytes;
    u32 lanes;          // generic form: lanes per lane group (a power of two, 4 .. 64)
    float c, scale;     // scale log2(e), rounded once from double; scale
};

// v_exp_f32: 2^x to 1 ulp, 0 for -inf (and for results under 2^-126)
__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }
// softmax.hip's conventions: a maximum of -inf (every score -inf, or no entry) shifts by 0, and
// a sum of 0 gives weights 0
__device__ __forceinline__ float shift_of(float m) { return m == -INFINITY ? 0.f : m; }
__device__ __forceinline__ float inverse_of(float s) { return s == 0.f ? 0.f : 1.0f / s; }

// LANES: lanes per lane group, compile-time (8, 16, 32, 64: rows of 128 .. 1024 bytes) or 0 =
// a.lanes (every other row size: multiples of 32 bytes from 64 on). Lanes past the K row or the
// V row idle for that operand. At most 64 VGPRs (k_softmax_rows' lesson: two resident workgroups
// of 16 waves)
template <int DT, int LANES>
__global__ __launch_bounds__(ATTN_WAVES * 64) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_attention(const AttnArgs a) {
    using E = Elem<DT>;
    constexpr int EPL = E::EPL;
    // gathered rows a lane group keeps in flight: 16 VGPRs of loads for fp32; the fp16 / bf16 forms
    // unpack 8 values per load and stay inside 64 VGPRs with two
    constexpr u32 ATTN_UNROLL = EPL == 4 ? 4 : 2;
    __shared__ float scores[ATTN_WAVES][ATTN_CHUNK];
    const u32 lane = threadIdx.x & 63u;
    // the wave's segment, wave-uniform (scalar loads of its descriptor, scalar loop counters)
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 segId = blockIdx.x * ATTN_WAVES + wave;
    if (segId >= a.nSegs) return;
    const SpmmSeg sg = a.segs[segId];
    const u32 L = LANES ? static_cast<u32>(LANES) : a.lanes;
    const u32 G = 64u / L;  // entries per instruction
    const u32 g = lane / L, l = lane % L;
    const bool liveK = l * 16u < a.kBytes, liveV = l * 16u < a.vBytes;
    float* score = scores[wave];

    float q[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) q[i] = 0.f;
    if (liveK)
        E::unpack(*reinterpret_cast<const uint4*>(a.Q + static_cast<size_t>(sg.dst) * a.kBytes + l * 16u), q);
    // a batch's column indices, one entry per lane. The first batch stays in a register for both
    // phases (a row of up to 64 entries reads its indices once); a later batch is loaded under
    // the gathers of the one before it, in each phase (4 bytes per entry from L2 against a
    // register per 64 entries of the chunk). Every lane takes part in the shuffles (an idle lane
    // may hold another's index); only the loads, the maximum and the sums are predicated
    auto batch = [&](u32 b0) {
        return b0 + lane < sg.count ? a.colidx[static_cast<size_t>(sg.first) + b0 + lane] : 0u;
    };
    const u32 cj0 = batch(0);
    auto row_of = [&](const char* X, u32 rowBytes, u32 col) {
        return *reinterpret_cast<const uint4*>(X + static_cast<size_t>(col) * rowBytes + l * 16u);
    };

    // ---- phase 1: scores and their maximum
    float m = -INFINITY;
    auto dot = [&](const uint4& w, bool valid, u32 slot) {
        float x[EPL];
        E::unpack(w, x);
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < EPL; ++i) d = __builtin_fmaf(q[i], x[i], d);
        for (u32 off = L >> 1; off >= 1u; off >>= 1) d += __shfl_xor(d, static_cast<int>(off));
        if (valid) {
            m = fmaxf(m, d);
            if (l == 0) score[slot] = d;
        }
    };
    for (u32 b0 = 0, cj = cj0; b0 < sg.count; b0 += 64u) {
        const u32 next = b0 + 64u < sg.count ? batch(b0 + 64u) : 0u;
        const u32 nb = min(64u, sg.count - b0);
        const u32 full = nb / G;  // steps in which every lane group has an entry
        u32 j = 0;
        for (; j + ATTN_UNROLL <= full; j += ATTN_UNROLL) {
            uint4 w[ATTN_UNROLL];
#pragma unroll
            for (u32 u = 0; u < ATTN_UNROLL; ++u) {
                const u32 col = __shfl(cj, static_cast<int>((j + u) * G + g));
                w[u] = liveK ? row_of(a.K, a.kBytes, col) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (u32 u = 0; u < ATTN_UNROLL; ++u) dot(w[u], true, b0 + (j + u) * G + g);
        }
        for (; j * G < nb; ++j) {  // the remaining steps; the last may be partly filled
            const u32 idx = j * G + g;
            const u32 col = __shfl(cj, static_cast<int>(idx & 63u));
            const bool valid = idx < nb;
            dot(liveK && valid ? row_of(a.K, a.kBytes, col) : make_uint4(0, 0, 0, 0), valid, b0 + idx);
        }
        cj = next;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    const float shift = shift_of(m);
    // the scores were written by each group's first lane and are read by all of its lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- phase 2: weights, their sum and the weighted V rows
    float ls = 0.f;
    float acc[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) acc[i] = 0.f;
    auto add = [&](const uint4& w, float p) {
        const float t = exp2_hw((p - shift) * a.c);
        ls += t;
        float x[EPL];
        E::unpack(w, x);
#pragma unroll
        for (int i = 0; i < EPL; ++i) acc[i] = __builtin_fmaf(t, x[i], acc[i]);
    };
    for (u32 b0 = 0, cj = cj0; b0 < sg.count; b0 += 64u) {
        const u32 next = b0 + 64u < sg.count ? batch(b0 + 64u) : 0u;
        const u32 nb = min(64u, sg.count - b0);
        const u32 full = nb / G;
        u32 j = 0;
        for (; j + ATTN_UNROLL <= full; j += ATTN_UNROLL) {
            uint4 w[ATTN_UNROLL];
            float p[ATTN_UNROLL];
#pragma unroll
            for (u32 u = 0; u < ATTN_UNROLL; ++u) {
                const u32 idx = (j + u) * G + g;
                const u32 col = __shfl(cj, static_cast<int>(idx));
                w[u] = liveV ? row_of(a.V, a.vBytes, col) : make_uint4(0, 0, 0, 0);
                p[u] = score[b0 + idx];
            }
#pragma unroll
            for (u32 u = 0; u < ATTN_UNROLL; ++u) add(w[u], p[u]);
        }
        for (; j * G < nb; ++j) {
            const u32 idx = j * G + g;
            const u32 col = __shfl(cj, static_cast<int>(idx & 63u));
            if (idx < nb) add(liveV ? row_of(a.V, a.vBytes, col) : make_uint4(0, 0, 0, 0), score[b0 + idx]);
        }
        cj = next;
    }
    // the groups in group order (group g held entries g, g + G, ... of the segment): every lane
    // ends with the same totals
    if (G > 1u) {
        auto total = [&](float v) {
            float t = __shfl(v, static_cast<int>(l));
            for (u32 gg = 1; gg < G; ++gg) t += __shfl(v, static_cast<int>(gg * L + l));
            return t;
        };
        ls = total(ls);
#pragma unroll
        for (int i = 0; i < EPL; ++i) acc[i] = total(acc[i]);
    }

    if (sg.part == SPMM_DIRECT) {
        const float inv = inverse_of(ls);
        if (g == 0 && liveV) {
            float* o = a.O + static_cast<size_t>(sg.dst) * a.Dv + static_cast<size_t>(l) * EPL;
#pragma unroll
            for (int i = 0; i < EPL; i += 4)
                *reinterpret_cast<float4*>(o + i) =
                    make_float4(acc[i] * inv, acc[i + 1] * inv, acc[i + 2] * inv, acc[i + 3] * inv);
        }
        if (lane == 0 && a.lse) a.lse[sg.dst] = m * a.scale + logf(ls);
    } else {
        if (g == 0 && liveV) {
            float* o = a.pacc + static_cast<size_t>(sg.part) * a.Dv + static_cast<size_t>(l) * EPL;
#pragma unroll
            for (int i = 0; i < EPL; i += 4)
                *reinterpret_cast<float4*>(o + i) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
        }
        if (lane == 0) {
            a.pml[2u * static_cast<size_t>(sg.part)] = m;
            a.pml[2u * static_cast<size_t>(sg.part) + 1u] = ls;
        }
    }
}

// a split row: M = max_s m_s, then every partial scaled once by f_s = 2^((m_s - M) c) (a rounded
// product each, never fused into the sum) and added in segment order; one thread per four columns
__global__ __launch_bounds__(256) void k_attention_reduce(const SpmmRed* reds, u32 nReds, const float* pacc,
                                                          const float* pml, float* O, float* lse, u32 Dv,
                                                          float c, float scale) {
#pragma clang fp contract(off)
    const u32 q4 = Dv / 4u;
    const size_t t = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= static_cast<size_t>(nReds) * q4) return;
    const SpmmRed r = reds[t / q4];
    const u32 q = static_cast<u32>(t % q4);
    const float* ml = pml + 2u * static_cast<size_t>(r.part0);
    const float4* p = reinterpret_cast<const float4*>(pacc + static_cast<size_t>(r.part0) * Dv) + q;
    float m = ml[0];
    for (u32 i = 1; i < r.nparts; ++i) m = fmaxf(m, ml[2u * i]);
    const float shift = shift_of(m);
    float ls = 0.f;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (u32 i = 0; i < r.nparts; ++i) {
        const float f = exp2_hw((ml[2u * i] - shift) * c);
        const float4 x = p[static_cast<size_t>(i) * q4];
        const float fl = f * ml[2u * i + 1u], fx = f * x.x, fy = f * x.y, fz = f * x.z, fw = f * x.w;
        ls = i ? ls + fl : fl;
        s.x = i ? s.x + fx : fx;
        s.y = i ? s.y + fy : fy;
        s.z = i ? s.z + fz : fz;
        s.w = i ? s.w + fw : fw;
    }
    const float inv = inverse_of(ls);
    reinterpret_cast<float4*>(O + static_cast<size_t>(r.dst) * Dv)[q] =
        make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
    if (q == 0 && lse) lse[r.dst] = m * scale + logf(ls);
}

using AttnFn = void (*)(const AttnArgs);

template <int DT>
AttnFn pick_attention(u32 rowBytes) {
    switch (rowBytes) {
        case 128: return k_attention<DT, 8>;
        case 256: return k_attention<DT, 16>;
        case 512: return k_attention<DT, 32>;
        case 1024: return k_attention<DT, 64>;
        default: return k_attention<DT, 0>;
    }
}

}  // namespace

// (attention_common.hpp: shared with attention_bwd.hip)
// the rules of the chain it replaces: D a positive multiple of 16 (fp32) or 32 (fp16 / bf16: what
// bsmr_sddmm takes), Dv a positive multiple of 16 (bsmr_spmm's K); and rows of at most 1024 bytes
int attn_validate_dims(const char* who, u32 D, u32 Dv, int dtype) {
    if (dtype != BSMR_F32 && dtype != BSMR_F16 && dtype != BSMR_BF16) {
        set_error(std::string(who) + ": dtype must be BSMR_F32, BSMR_F16 or BSMR_BF16");
        return BSMR_ERR_UNSUPPORTED;
    }
    const u32 mult = dtype == BSMR_F32 ? 16u : 32u, esz = dtype == BSMR_F32 ? 4u : 2u;
    if (D == 0 || D % mult != 0 || Dv == 0 || Dv % 16u != 0 || std::max(D, Dv) > ATTN_MAX_ROW_BYTES / esz) {
        set_error(std::string(who) + ": D must be a positive multiple of " + std::to_string(mult) +
                  " and Dv of 16, with rows of at most " + std::to_string(ATTN_MAX_ROW_BYTES) + " bytes");
        return BSMR_ERR_UNSUPPORTED;
    }
    return BSMR_OK;
}

// the prepare calls carry no dtype: what some dtype accepts
int attn_validate_prepare_dims(const char* who, u32 D, u32 Dv) {
    if (attn_validate_dims(who, D, Dv, BSMR_F32) == BSMR_OK) return BSMR_OK;
    return attn_validate_dims(who, D, Dv, BSMR_F16);
}

// bsmr_softmax's rule: the exponent factor is rounded once from double
int attn_validate_scale(const char* who, float scale, float* c) {
    *c = static_cast<float>(static_cast<double>(scale) * 1.4426950408889634);
    if (!(scale > 0.f) || !std::isfinite(scale) || !std::isfinite(*c)) {
        set_error(std::string(who) + ": scale must be finite and > 0 (and scale * log2(e) finite)");
        return BSMR_ERR_INVALID;
    }
    return BSMR_OK;
}

u32 attn_forward_chunk() { return ATTN_CHUNK; }

int attn_row_lists(const Plan& p, u32 chunk, const char* who, SpmmLists& L) {
    const hipStream_t s = p.stream;
    std::vector<u32> hrp, hci, hrows;
    BSMR_CHECK(p.rowptr.download(hrp, s));
    BSMR_CHECK(p.colidx.download(hci, s));
    // rows in the plan's reordered order: a workgroup's waves share a panel's columns
    BSMR_CHECK(p.rows.download(hrows, s));
    hrows.resize(std::min<size_t>(hrows.size(), p.R));
    SpmmIn in;
    in.M = p.M;
    in.N = p.N;
    in.nnz = p.nnz;
    in.rowptr = hrp.data();
    in.colidx = hci.data();
    in.side = 1;
    in.chunk = chunk;
    in.order = hrows.data();
    in.norder = static_cast<u32>(hrows.size());
    std::string err;
    if (spmm_lists(in, L, err)) {
        set_error(std::string(who) + ": " + err);
        return BSMR_ERR_INVALID;
    }
    if (L.nSegs > (1ull << 31)) {
        set_error(std::string(who) + ": more than 2^31 segments");
        return BSMR_ERR_UNSUPPORTED;
    }
    return BSMR_OK;
}

namespace {

bool attention_ready(const Plan::AttentionState& S, u32 Dv) {
    return S.built && (S.partials == 0 || S.scratchDv >= Dv);
}

// build the segment list (once) and size the scratch for Dv; layout_mu held. Synchronous on the
// plan's stream.
int build_attention(const Plan& p, u32 Dv) {
    Plan::AttentionState& S = p.attention;
    const hipStream_t s = p.stream;
    if (!S.built) {
        SpmmLists L;
        BSMR_CHECK(attn_row_lists(p, ATTN_CHUNK, "bsmr_plan_prepare_attention", L));
        // (on side 1 L.src is colidx and L.vpos the identity: the plan's own colidx serves)
        BSMR_CHECK(S.segs.upload(L.segs.data(), L.segs.size(), s));
        BSMR_CHECK(S.reds.upload(L.reds.data(), L.reds.size(), s));
        BSMR_HIP(hipStreamSynchronize(s));
        S.nSegs = static_cast<u32>(L.nSegs);
        S.nReds = static_cast<u32>(L.reds.size());
        S.splitRows = L.splitDsts;
        S.partials = L.partials;
        S.maxRow = L.maxList;
        S.scratchDv = 0;
        S.built = true;
    }
    if (S.partials != 0 && S.scratchDv < Dv) {
        S.scratchDv = 0;
        BSMR_CHECK(S.scratch.alloc(static_cast<size_t>(S.partials) * (Dv + 2u)));
        S.scratchDv = Dv;
    }
    return BSMR_OK;
}

}  // namespace
}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_attention(const bsmr_plan* plan, const void* dQ, const void* dK, const void* dV, uint32_t D,
                              uint32_t Dv, int dtype, float scale, float* dO, float* dLse, void* stream) {
    const char* who = "bsmr_attention";
    if (!plan) {
        set_error("bsmr_attention: null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dQ || !dK || !dV || !dO) {
        set_error("bsmr_attention: null device pointer");
        return BSMR_ERR_INVALID;
    }
    if (!attn_aligned16(dQ) || !attn_aligned16(dK) || !attn_aligned16(dV) || !attn_aligned16(dO) ||
        (reinterpret_cast<uintptr_t>(dLse) & 3u)) {
        set_error("bsmr_attention: dQ, dK, dV and dO must be 16-byte aligned");
        return BSMR_ERR_INVALID;
    }
    float c;
    BSMR_CHECK(attn_validate_scale(who, scale, &c));
    BSMR_CHECK(attn_validate_dims(who, D, Dv, dtype));
    const Plan& p = plan->p;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Plan::AttentionState& S = p.attention;
    AttnArgs a{};
    const SpmmRed* reds = nullptr;
    u32 nReds = 0, partials = 0;
    {
        std::lock_guard<std::mutex> g(p.layout_mu);
        if (!attention_ready(S, Dv)) {
            const LaunchSite at{s, who, "bsmr_plan_prepare_attention", D, dtype};
            const int st = lazy_build_guard(at);
            if (st == BSMR_ERR_NOT_PREPARED)  // (the guard's own message names a (K, dtype) layout)
                set_error("bsmr_attention: stream is capturing and the attention lists (or their scratch for Dv = " +
                          std::to_string(Dv) + ") are not built; call bsmr_plan_prepare_attention first");
            BSMR_CHECK(st);
            BSMR_CHECK(build_attention(p, Dv));
        }
        a.segs = S.segs.data();
        a.nSegs = S.nSegs;
        a.pacc = S.scratch.data();
        reds = S.reds.data();
        nReds = S.nReds;
        partials = S.partials;
    }
    const u32 esz = dtype == BSMR_F32 ? 4u : 2u;
    a.pml = a.pacc ? a.pacc + static_cast<size_t>(partials) * Dv : nullptr;
    a.colidx = p.colidx.data();
    a.Q = static_cast<const char*>(dQ);
    a.K = static_cast<const char*>(dK);
    a.V = static_cast<const char*>(dV);
    a.O = dO;
    a.lse = dLse;
    a.Dv = Dv;
    a.kBytes = D * esz;
    a.vBytes = Dv * esz;
    a.c = c;
    a.scale = scale;
    const u32 rowBytes = std::max(a.kBytes, a.vBytes);
    a.lanes = 4;
    while (a.lanes * 16u < rowBytes) a.lanes <<= 1;
    const AttnFn fn = dtype == BSMR_F32   ? pick_attention<BSMR_F32>(rowBytes)
                      : dtype == BSMR_F16 ? pick_attention<BSMR_F16>(rowBytes)
                                          : pick_attention<BSMR_BF16>(rowBytes);
    if (a.nSegs) {
        const u32 grid = (a.nSegs + ATTN_WAVES - 1) / ATTN_WAVES;
        hipLaunchKernelGGL(fn, dim3(grid), dim3(ATTN_WAVES * 64), 0, s, a);
        BSMR_HIP(hipGetLastError());
    }
    if (nReds) {
        const size_t threads = static_cast<size_t>(nReds) * (Dv / 4u);
        hipLaunchKernelGGL(k_attention_reduce, dim3(static_cast<u32>((threads + 255) / 256)), dim3(256), 0, s, reds,
                           nReds, a.pacc, a.pml, dO, dLse, Dv, c, scale);
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

extern "C" int bsmr_plan_prepare_attention(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    if (!plan) {
        set_error("bsmr_plan_prepare_attention: null plan");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(attn_validate_prepare_dims("bsmr_plan_prepare_attention", D, Dv));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_attention(plan->p, Dv);
}

extern "C" int bsmr_plan_attention_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    if (!plan) {
        set_error("bsmr_plan_attention_prepared: null plan");
        return 0;
    }
    if (attn_validate_prepare_dims("bsmr_plan_attention_prepared", D, Dv) != BSMR_OK) return 0;
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return attention_ready(plan->p.attention, Dv) ? 1 : 0;
}

extern "C" int bsmr_plan_attention_stats(const bsmr_plan* plan, bsmr_attention_stats* out) {
    if (!plan || !out) {
        set_error("bsmr_plan_attention_stats: null argument");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    const Plan::AttentionState& S = p.attention;
    *out = bsmr_attention_stats{};
    out->chunk = ATTN_CHUNK;
    if (S.built) {
        out->segments = S.nSegs;
        out->split_rows = S.splitRows;
        out->partials = S.partials;
        out->max_row = S.maxRow;
    }
    return BSMR_OK;
}

extern "C" void bsmr_attention_limits(uint32_t* chunk, uint32_t* max_row_bytes) {
    if (chunk) *chunk = ATTN_CHUNK;
    if (max_row_bytes) *max_row_bytes = ATTN_MAX_ROW_BYTES;
}
