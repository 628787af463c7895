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
//
// Batch and heads (bsmr_attention_heads): the same kernels over Z = batches x heads slices of one
// pattern in one grid. blockIdx.x stays the segment index, so that a slice's workgroups are
// dispatched together; blockIdx.y is the head and blockIdx.z the batch. Every operand carries a
// batch and a head stride (64-bit, bytes) and a row stride (32-bit, bytes); the slice's base
// pointers are wave-uniform and computed once at kernel entry in scalar registers. LSE is dense
// (batches, heads, M) and the scratch is per slice. bsmr_attention is the one-slice, dense-stride
// case of the same launch code.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "attention_common.hpp"
#include "attention_layout.hpp"
#include "plan.hpp"
#include "row_elems.hpp"
#include "seg_walk.hpp"  // exp2_hw
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
    const char* Q;      // per slice M rows of kBytes, qRow bytes apart
    const char* K;      // per slice N rows of kBytes, kRow bytes apart
    const char* V;      // per slice N rows of vBytes, vRow bytes apart
    char* O;            // per slice M rows of Dv floats, oRow bytes apart
    float* lse;         // slices x M, or null
    float* pacc;        // slices x partial slots x Dv
    float* pml;         // behind them: slices x partial slots x (m, l); both 16-byte aligned per slice
    u64 qB, qH, kB, kH, vB, vH, oB, oH;  // batch and head strides in bytes
    u32 partials;       // partial slots per slice
    u32 qRow, kRow, vRow, oRow;  // row strides in bytes
    u32 heads, M;
    u32 nSegs, Dv, kBytes, vBytes;
    u32 lanes;          // generic form: lanes per lane group (a power of two, 4 .. 64)
    float c, scale;     // scale log2(e), rounded once from double; scale
};

// softmax.hip's conventions: a maximum of -inf (every score -inf, or no entry) shifts by 0, and
// a sum of 0 gives weights 0
__device__ __forceinline__ float shift_of(float m) { return m == -INFINITY ? 0.f : m; }
__device__ __forceinline__ float inverse_of(float s) { return s == 0.f ? 0.f : 1.0f / s; }

// LANES: lanes per lane group, compile-time (8, 16, 32, 64: rows of 128 .. 1024 bytes) or 0 =
// a.lanes (every other row size: multiples of 32 bytes from 64 on). Lanes past the K row or the
// V row idle for that operand. At most 64 VGPRs (k_softmax_rows' lesson: two resident workgroups
// of 16 waves)
// SLICES: false is the one-slice instantiation that bsmr_attention keeps (no slice arithmetic, no
// branch: the shared form measured 0.3 us slower on C2)
template <int DT, int LANES, bool SLICES>
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
    // the slice (head blockIdx.y of batch blockIdx.z): wave-uniform 64-bit bases, scalar registers
    size_t slice = 0;
    const char *Qs = a.Q, *Ks = a.K, *Vs = a.V;
    char* Os = a.O;
    if (SLICES) {
        const u32 head = blockIdx.y, bat = blockIdx.z;
        slice = static_cast<size_t>(bat) * a.heads + head;
        Qs += bat * a.qB + head * a.qH;
        Ks += bat * a.kB + head * a.kH;
        Vs += bat * a.vB + head * a.vH;
        Os += bat * a.oB + head * a.oH;
    }
    const u32 L = LANES ? static_cast<u32>(LANES) : a.lanes;
    const u32 G = 64u / L;  // entries per instruction
    const u32 g = lane / L, l = lane % L;
    const bool liveK = l * 16u < a.kBytes, liveV = l * 16u < a.vBytes;
    float* score = scores[wave];

    float q[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) q[i] = 0.f;
    if (liveK)
        E::unpack(*reinterpret_cast<const uint4*>(Qs + static_cast<size_t>(sg.dst) * a.qRow + l * 16u), q);
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
                w[u] = liveK ? row_of(Ks, a.kRow, col) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (u32 u = 0; u < ATTN_UNROLL; ++u) dot(w[u], true, b0 + (j + u) * G + g);
        }
        for (; j * G < nb; ++j) {  // the remaining steps; the last may be partly filled
            const u32 idx = j * G + g;
            const u32 col = __shfl(cj, static_cast<int>(idx & 63u));
            const bool valid = idx < nb;
            dot(liveK && valid ? row_of(Ks, a.kRow, col) : make_uint4(0, 0, 0, 0), valid, b0 + idx);
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
                w[u] = liveV ? row_of(Vs, a.vRow, col) : make_uint4(0, 0, 0, 0);
                p[u] = score[b0 + idx];
            }
#pragma unroll
            for (u32 u = 0; u < ATTN_UNROLL; ++u) add(w[u], p[u]);
        }
        for (; j * G < nb; ++j) {
            const u32 idx = j * G + g;
            const u32 col = __shfl(cj, static_cast<int>(idx & 63u));
            if (idx < nb) add(liveV ? row_of(Vs, a.vRow, col) : make_uint4(0, 0, 0, 0), score[b0 + idx]);
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
            float* o = reinterpret_cast<float*>(Os + static_cast<size_t>(sg.dst) * a.oRow) + static_cast<size_t>(l) * EPL;
#pragma unroll
            for (int i = 0; i < EPL; i += 4)
                *reinterpret_cast<float4*>(o + i) =
                    make_float4(acc[i] * inv, acc[i + 1] * inv, acc[i + 2] * inv, acc[i + 3] * inv);
        }
        if (lane == 0 && a.lse) a.lse[slice * a.M + sg.dst] = m * a.scale + logf(ls);
    } else {
        if (g == 0 && liveV) {
            float* o = a.pacc + (slice * a.partials + sg.part) * a.Dv + static_cast<size_t>(l) * EPL;
#pragma unroll
            for (int i = 0; i < EPL; i += 4)
                *reinterpret_cast<float4*>(o + i) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
        }
        if (lane == 0) {
            float* ml = a.pml + 2u * (slice * a.partials + sg.part);
            ml[0] = m;
            ml[1] = ls;
        }
    }
}

// a split row: M = max_s m_s, then every partial scaled once by f_s = 2^((m_s - M) c) (a rounded
// product each, never fused into the sum) and added in segment order; one thread per four columns
template <bool SLICES>
__global__ __launch_bounds__(256) void k_attention_reduce(const AttnArgs a, const SpmmRed* reds, u32 nReds) {
#pragma clang fp contract(off)
    const u32 Dv = a.Dv;
    const float c = a.c, scale = a.scale;
    size_t slice = 0;
    char* O = a.O;
    if (SLICES) {
        const u32 head = blockIdx.y, bat = blockIdx.z;
        slice = static_cast<size_t>(bat) * a.heads + head;
        O += bat * a.oB + head * a.oH;
    }
    const float* pacc = a.pacc + slice * a.partials * Dv;
    const float* pml = a.pml + 2u * slice * a.partials;
    float* lse = a.lse ? a.lse + slice * a.M : nullptr;
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
    reinterpret_cast<float4*>(O + static_cast<size_t>(r.dst) * a.oRow)[q] =
        make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
    if (q == 0 && lse) lse[r.dst] = m * scale + logf(ls);
}

using AttnFn = void (*)(const AttnArgs);

template <int DT, bool SLICES>
AttnFn pick_attention(u32 rowBytes) {
    switch (rowBytes) {
        case 128: return k_attention<DT, 8, SLICES>;
        case 256: return k_attention<DT, 16, SLICES>;
        case 512: return k_attention<DT, 32, SLICES>;
        case 1024: return k_attention<DT, 64, SLICES>;
        default: return k_attention<DT, 0, SLICES>;
    }
}

template <bool SLICES>
AttnFn pick_attention(int dtype, u32 rowBytes) {
    return dtype == BSMR_F32   ? pick_attention<BSMR_F32, SLICES>(rowBytes)
           : dtype == BSMR_F16 ? pick_attention<BSMR_F16, SLICES>(rowBytes)
                               : pick_attention<BSMR_BF16, SLICES>(rowBytes);
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

size_t attention_scratch_floats(const Plan::AttentionState& S, u32 Dv, u32 slices) {
    return attn_sat_mul(slices, S.partials, Dv + 2u);
}

bool attention_ready(const Plan::AttentionState& S, u32 Dv, u32 slices) {
    // (DevBuf holds a size only with its memory: a failed grow leaves the old buffer and its size)
    return S.built && S.scratch.size() >= attention_scratch_floats(S, Dv, slices);
}

// build the segment list (once) and size the per-slice scratch for (Dv, slices): it grows and
// never shrinks; layout_mu held. Synchronous on the plan's stream.
int build_attention(const Plan& p, u32 Dv, u32 slices, const char* who) {
    Plan::AttentionState& S = p.attention;
    const hipStream_t s = p.stream;
    if (!S.built) {
        SpmmLists L;
        BSMR_CHECK(attn_row_lists(p, ATTN_CHUNK, who, L));
        // (on side 1 L.src is colidx and L.vpos the identity: the plan's own colidx serves)
        BSMR_CHECK(S.segs.upload(L.segs.data(), L.segs.size(), s));
        BSMR_CHECK(S.reds.upload(L.reds.data(), L.reds.size(), s));
        BSMR_HIP(hipStreamSynchronize(s));
        S.nSegs = static_cast<u32>(L.nSegs);
        S.nReds = static_cast<u32>(L.reds.size());
        S.splitRows = L.splitDsts;
        S.partials = L.partials;
        S.maxRow = L.maxList;
        S.built = true;
    }
    return S.scratch.grow(attention_scratch_floats(S, Dv, slices));
}

// the launches of bsmr_attention and bsmr_attention_heads, arguments already validated: `who` and
// `prep` name the entry point and its prepare call in errors
int attention_launch(const char* who, const char* prep, const bsmr_plan* plan, u32 batches, u32 heads,
                     const bsmr_attention_operand& Q, const bsmr_attention_operand& K, const bsmr_attention_operand& V,
                     u32 D, u32 Dv, int dtype, float scale, float c, const bsmr_attention_operand& O, float* dLse,
                     void* stream) {
    const Plan& p = plan->p;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Plan::AttentionState& S = p.attention;
    const u32 slices = batches * heads;  // (both at most 65535)
    AttnArgs a{};
    const SpmmRed* reds = nullptr;
    u32 nReds = 0, partials = 0;
    {
        std::lock_guard<std::mutex> g(p.layout_mu);
        if (!attention_ready(S, Dv, slices)) {
            const LaunchSite at{s, who, prep, D, dtype};
            const int st = lazy_build_guard(at);
            if (st == BSMR_ERR_NOT_PREPARED)  // (the guard's own message names a (K, dtype) layout)
                set_error(std::string(who) + ": stream is capturing and the attention lists (or their scratch for Dv = " +
                          std::to_string(Dv) + (slices > 1 ? ", " + std::to_string(slices) + " slices" : std::string()) +
                          ") are not built; call " + prep + " first");
            BSMR_CHECK(st);
            BSMR_CHECK(build_attention(p, Dv, slices, prep));
        }
        a.segs = S.segs.data();
        a.nSegs = S.nSegs;
        a.pacc = S.scratch.data();
        reds = S.reds.data();
        nReds = S.nReds;
        partials = S.partials;
    }
    const u32 esz = dtype == BSMR_F32 ? 4u : 2u;
    a.pml = a.pacc ? a.pacc + static_cast<size_t>(slices) * partials * Dv : nullptr;
    a.partials = partials;
    a.colidx = p.colidx.data();
    const AttnOpBytes q = attn_op_bytes(&Q, batches, heads, p.M, esz), k = attn_op_bytes(&K, batches, heads, p.N, esz),
                      v = attn_op_bytes(&V, batches, heads, p.N, esz), o = attn_op_bytes(&O, batches, heads, p.M, 4u);
    a.Q = q.ptr, a.qB = q.batch, a.qH = q.head, a.qRow = q.row;
    a.K = k.ptr, a.kB = k.batch, a.kH = k.head, a.kRow = k.row;
    a.V = v.ptr, a.vB = v.batch, a.vH = v.head, a.vRow = v.row;
    a.O = o.ptr, a.oB = o.batch, a.oH = o.head, a.oRow = o.row;
    a.lse = dLse;
    a.heads = heads;
    a.M = p.M;
    a.Dv = Dv;
    a.kBytes = D * esz;
    a.vBytes = Dv * esz;
    a.c = c;
    a.scale = scale;
    const u32 rowBytes = std::max(a.kBytes, a.vBytes);
    a.lanes = attn_lanes(rowBytes);
    const AttnFn fn = slices > 1 ? pick_attention<true>(dtype, rowBytes) : pick_attention<false>(dtype, rowBytes);
    if (a.nSegs) {
        const u32 grid = (a.nSegs + ATTN_WAVES - 1) / ATTN_WAVES;
        hipLaunchKernelGGL(fn, dim3(grid, heads, batches), dim3(ATTN_WAVES * 64), 0, s, a);
        BSMR_HIP(hipGetLastError());
    }
    if (nReds) {
        const size_t threads = static_cast<size_t>(nReds) * (Dv / 4u);
        const dim3 rgrid(static_cast<u32>((threads + 255) / 256), heads, batches);
        if (slices > 1)
            hipLaunchKernelGGL(k_attention_reduce<true>, rgrid, dim3(256), 0, s, a, reds, nReds);
        else
            hipLaunchKernelGGL(k_attention_reduce<false>, rgrid, dim3(256), 0, s, a, reds, nReds);
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

}  // namespace

// (attention_common.hpp)
int attn_check_slices(const char* who, u32 slices) {
    if (slices == 0 || slices > BSMR_ATTENTION_MAX_BATCHES * static_cast<u64>(BSMR_ATTENTION_MAX_HEADS)) {
        set_error(std::string(who) + ": slices must be 1 .. BSMR_ATTENTION_MAX_BATCHES x BSMR_ATTENTION_MAX_HEADS");
        return BSMR_ERR_INVALID;
    }
    return BSMR_OK;
}

// (attention_common.hpp) one operand of a heads call against the layout rules
int attn_check_operand(const char* who, const char* name, const bsmr_attention_operand* op, u32 batches, u32 heads,
                       u32 rows, u32 width, u32 esz, bool is_output) {
    std::string err;
    if (attention_layout_check(op, batches, heads, rows, width, esz, is_output, err)) {
        set_error(std::string(who) + ": " + name + ": " + err);
        return BSMR_ERR_INVALID;
    }
    return BSMR_OK;
}

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
    return attention_launch(who, "bsmr_plan_prepare_attention", plan, 1, 1, attention_dense_operand(dQ, 1, p.M, D),
                            attention_dense_operand(dK, 1, p.N, D), attention_dense_operand(dV, 1, p.N, Dv), D, Dv, dtype,
                            scale, c, attention_dense_operand(dO, 1, p.M, Dv), dLse, stream);
}

extern "C" int bsmr_attention_heads(const bsmr_plan* plan, uint32_t batches, uint32_t heads,
                                    const bsmr_attention_operand* Q, const bsmr_attention_operand* K,
                                    const bsmr_attention_operand* V, uint32_t D, uint32_t Dv, int dtype, float scale,
                                    const bsmr_attention_operand* O, float* dLse, void* stream) {
    const char* who = "bsmr_attention_heads";
    if (!plan) {
        set_error("bsmr_attention_heads: null plan");
        return BSMR_ERR_INVALID;
    }
    if (reinterpret_cast<uintptr_t>(dLse) & 3u) {
        set_error("bsmr_attention_heads: dLse must be 4-byte aligned");
        return BSMR_ERR_INVALID;
    }
    float c;
    BSMR_CHECK(attn_validate_scale(who, scale, &c));
    BSMR_CHECK(attn_validate_dims(who, D, Dv, dtype));
    const Plan& p = plan->p;
    const u32 esz = dtype == BSMR_F32 ? 4u : 2u;
    BSMR_CHECK(attn_check_operand(who, "Q", Q, batches, heads, p.M, D, esz, false));
    BSMR_CHECK(attn_check_operand(who, "K", K, batches, heads, p.N, D, esz, false));
    BSMR_CHECK(attn_check_operand(who, "V", V, batches, heads, p.N, Dv, esz, false));
    BSMR_CHECK(attn_check_operand(who, "O", O, batches, heads, p.M, Dv, 4u, true));
    return attention_launch(who, "bsmr_plan_prepare_attention_heads", plan, batches, heads, *Q, *K, *V, D, Dv, dtype, scale,
                            c, *O, dLse, stream);
}

extern "C" int bsmr_attention_layout_check(const bsmr_attention_operand* op, uint32_t batches, uint32_t heads,
                                           uint32_t rows, uint32_t width, uint32_t elem_bytes, int is_output) {
    return attn_check_operand("bsmr_attention_layout_check", "operand", op, batches, heads, rows, width, elem_bytes,
                              is_output != 0);
}

extern "C" int bsmr_plan_prepare_attention(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    if (!plan) {
        set_error("bsmr_plan_prepare_attention: null plan");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(attn_validate_prepare_dims("bsmr_plan_prepare_attention", D, Dv));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_attention(plan->p, Dv, 1, "bsmr_plan_prepare_attention");
}

extern "C" int bsmr_plan_attention_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    if (!plan) {
        set_error("bsmr_plan_attention_prepared: null plan");
        return 0;
    }
    if (attn_validate_prepare_dims("bsmr_plan_attention_prepared", D, Dv) != BSMR_OK) return 0;
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return attention_ready(plan->p.attention, Dv, 1) ? 1 : 0;
}

extern "C" int bsmr_plan_prepare_attention_heads(const bsmr_plan* plan, uint32_t D, uint32_t Dv, uint32_t slices) {
    const char* who = "bsmr_plan_prepare_attention_heads";
    if (!plan) {
        set_error("bsmr_plan_prepare_attention_heads: null plan");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(attn_check_slices(who, slices));
    BSMR_CHECK(attn_validate_prepare_dims(who, D, Dv));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_attention(plan->p, Dv, slices, who);
}

extern "C" int bsmr_plan_attention_heads_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv, uint32_t slices) {
    const char* who = "bsmr_plan_attention_heads_prepared";
    if (!plan) {
        set_error("bsmr_plan_attention_heads_prepared: null plan");
        return 0;
    }
    if (attn_check_slices(who, slices) != BSMR_OK || attn_validate_prepare_dims(who, D, Dv) != BSMR_OK) return 0;
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return attention_ready(plan->p.attention, Dv, slices) ? 1 : 0;
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
