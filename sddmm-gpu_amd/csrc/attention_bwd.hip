// attention_bwd.hip — fused sparse attention backward for gfx950 (bsmr_attention_backward):
//
//   GQ[i,:] = sum_e dp_e K[j_e,:]   GK[j,:] = sum_{e in column j} dp_e Q[i_e,:]   GV[j,:] = sum w_e GO[i_e,:]
//   p_e = dot(Q[i,:], K[j,:]),  w_e = 2^((p_e scale - LSE[i]) log2e),  g_e = dot(GO[i,:], V[j,:]),
//   delta_i = dot(GO[i,:], O[i,:]),  dp_e = (w_e (g_e - delta_i)) scale
//
// from Q, K, V, O, GO = dL/dO and the forward's LSE, without an nnz-sized tensor: both sides
// compute p, w, g and dp per entry in registers, in one pass (LSE already holds the row's shift, so
// there is no maximum and no rescale). At most five launches:
//   k_attention_bwd_delta   delta (M floats of plan-owned scratch), one lane group per row;
//   k_attention_bwd_rows    one wave per segment of a row (the forward's lists): Q[i], GO[i], LSE[i]
//                           and delta_i in registers, K[j] and V[j] gathered per entry, GQ accumulated;
//   k_attention_bwd_cols    one wave per segment of a column (spmm_lists at side 2): K[j] and V[j] in
//                           registers, Q[i], GO[i], LSE[i] and delta_i gathered per entry, GK and GV;
//   k_attention_bwd_reduce  after either, the partial rows of split destinations added in segment
//                           order.
// The forward's lane layout: L = max(D, Dv) sizeof(T) / 16 lanes (rounded up to a power of two)
// cover a row with 16-byte loads, a lane owns the same element indices of every operand (its fp32
// GO / O elements are one or two 16-byte loads), and the 64 / L lane groups take consecutive
// entries. A dot product is the forward's: the lane's FMA chain in element order from 0, then the
// xor butterfly from L / 2 down to 1; delta uses the same order, so that g - delta cancels exactly
// where O is a V row. A group accumulates in entry order, one FMA per (entry, element); the groups
// are added in group order and the partials in segment order. fp32 throughout, no atomics: the
// order is a function of the destination's list length, D, Dv and the dtype alone.
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

// entries per segment of a row and of a column; macros so that an A/B build can override them
// (-DATTN_BWD_ROW_CHUNK=..., -DATTN_BWD_COL_CHUNK=...). Both start at the forward's 256
#ifndef ATTN_BWD_ROW_CHUNK
#define ATTN_BWD_ROW_CHUNK 256
#endif
#ifndef ATTN_BWD_COL_CHUNK
#define ATTN_BWD_COL_CHUNK 256
#endif
static_assert(ATTN_BWD_ROW_CHUNK >= 1 && ATTN_BWD_COL_CHUNK >= 1, "a segment holds an entry");
constexpr u32 ABW_WAVES = 16;  // waves (segments) per workgroup, as k_attention
constexpr u32 ABW_UNROLL = 2;  // entries a lane group keeps in flight (two gathered rows each)
constexpr float LOG2E_F = 1.44269504088896340736f;

struct BwdArgs {
    const SpmmSeg* segs;
    const u32* idx;      // rows side: the plan's colidx; columns side: the row of every entry
    const char* Q;       // M rows of kBytes
    const char* K;       // N rows of kBytes
    const char* V;       // N rows of vBytes
    const float* GO;     // M x Dv
    const float* lse;    // M
    const float* delta;  // M
    float* Y0;           // rows side: GQ (M x D); columns side: GK (N x D) or null
    float* Y1;           // columns side: GV (N x Dv) or null
    float* P0;           // partial slots x D
    float* P1;           // columns side: partial slots x Dv
    u32 nSegs, D, Dv, kBytes, vBytes;
    u32 lanes;           // generic form: lanes per lane group (a power of two, 4 .. 64)
    float scale;
};

// v_exp_f32: 2^x to 1 ulp, 0 for -inf (and for results under 2^-126)
__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }

// the entry's weight and score gradient, every product and difference rounded on its own: the
// exponent is (p scale - LSE) log2e, so a score that equals LSE bit for bit has weight exactly 1
__device__ __forceinline__ void weight_of(float p, float g, float lse, float dl, float scale, float& w, float& dp) {
#pragma clang fp contract(off)
    const float x = p * scale;
    const float d = x - lse;
    const float t = d * LOG2E_F;
    w = lse == -INFINITY ? 0.f : exp2_hw(t);
    const float gd = g - dl;
    const float wg = w * gd;
    dp = wg * scale;
}

template <int EPL>
__device__ __forceinline__ float group_dot(const float* a, const float* b, u32 L) {
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < EPL; ++i) d = __builtin_fmaf(a[i], b[i], d);
    for (u32 off = L >> 1; off >= 1u; off >>= 1) d += __shfl_xor(d, static_cast<int>(off));
    return d;
}

// EPL fp32 values of a row of `cols` floats, from element l EPL on
template <int EPL>
__device__ __forceinline__ void load_f32(const float* X, size_t row, u32 cols, u32 l, float* x) {
    const float4* p = reinterpret_cast<const float4*>(X + row * cols + static_cast<size_t>(l) * EPL);
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

// the lane groups in group order (group g held entries g, g + G, ... of the segment): every lane
// ends with the same totals
template <int EPL>
__device__ __forceinline__ void group_total(float* acc, u32 L, u32 G, u32 l) {
    if (G <= 1u) return;
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        float t = __shfl(acc[i], static_cast<int>(l));
#pragma unroll 1  // (unrolled, the 64 / L - 1 shuffles of every accumulator are all hoisted: spills at L = 8)
        for (u32 gg = 1; gg < G; ++gg) t += __shfl(acc[i], static_cast<int>(gg * L + l));
        acc[i] = t;
    }
}

// delta_i = dot(GO[i,:], O[i,:]) in the lane order of g_e: EPL elements per lane, L lanes per row,
// 64 / L rows per wave, four waves per workgroup
template <int EPL>
__global__ __launch_bounds__(256) void k_attention_bwd_delta(const float* GO, const float* O, float* delta, u32 M,
                                                             u32 Dv, u32 L) {
    const u32 lane = threadIdx.x & 63u;
    const u32 G = 64u / L, g = lane / L, l = lane % L;
    const size_t row = (static_cast<size_t>(blockIdx.x) * 4u + (threadIdx.x >> 6)) * G + g;
    const bool live = row < M && l * static_cast<u32>(EPL) < Dv;
    float a[EPL], b[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) a[i] = b[i] = 0.f;
    if (live) {
        load_f32<EPL>(GO, row, Dv, l, a);
        load_f32<EPL>(O, row, Dv, l, b);
    }
    const float d = group_dot<EPL>(a, b, L);
    if (row < M && l == 0) delta[row] = d;
}

// LANES: lanes per lane group, compile-time (8, 16, 32, 64: rows of 128 .. 1024 bytes) or 0 =
// a.lanes (every other row size). Lanes past the K row or the V row idle for that operand
template <int DT, int LANES>
__global__ __launch_bounds__(ABW_WAVES * 64) void k_attention_bwd_rows(const BwdArgs a) {
    using E = Elem<DT>;
    constexpr int EPL = E::EPL;
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 segId = blockIdx.x * ABW_WAVES + wave;
    if (segId >= a.nSegs) return;
    const SpmmSeg sg = a.segs[segId];
    const u32 L = LANES ? static_cast<u32>(LANES) : a.lanes;
    const u32 G = 64u / L;
    const u32 g = lane / L, l = lane % L;
    const bool liveK = l * 16u < a.kBytes, liveV = l * 16u < a.vBytes;
    const size_t row = sg.dst;

    float q[EPL], go[EPL], acc[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) q[i] = go[i] = acc[i] = 0.f;
    if (liveK) E::unpack(*reinterpret_cast<const uint4*>(a.Q + row * a.kBytes + l * 16u), q);
    if (liveV) load_f32<EPL>(a.GO, row, a.Dv, l, go);
    const float lse = a.lse[row], dl = a.delta[row];

    auto batch = [&](u32 b0) {
        return b0 + lane < sg.count ? a.idx[static_cast<size_t>(sg.first) + b0 + lane] : 0u;
    };
    auto row_of = [&](const char* X, u32 rowBytes, u32 col) {
        return *reinterpret_cast<const uint4*>(X + static_cast<size_t>(col) * rowBytes + l * 16u);
    };
    const uint4 zero = make_uint4(0, 0, 0, 0);
    // every lane takes part in the shuffles; only the loads and the FMAs into acc are predicated
    auto entry = [&](const uint4& kw, const uint4& vw, bool valid) {
        float kx[EPL], vx[EPL];
        E::unpack(kw, kx);
        E::unpack(vw, vx);
        const float p = group_dot<EPL>(q, kx, L);
        const float gg = group_dot<EPL>(go, vx, L);
        float w, dp;
        weight_of(p, gg, lse, dl, a.scale, w, dp);
        if (valid) {
#pragma unroll
            for (int i = 0; i < EPL; ++i) acc[i] = __builtin_fmaf(dp, kx[i], acc[i]);
        }
    };
    u32 cj = batch(0);
    for (u32 b0 = 0; b0 < sg.count; b0 += 64u) {
        const u32 next = b0 + 64u < sg.count ? batch(b0 + 64u) : 0u;
        const u32 nb = min(64u, sg.count - b0);
        const u32 full = nb / G;  // steps in which every lane group has an entry
        u32 j = 0;
        for (; j + ABW_UNROLL <= full; j += ABW_UNROLL) {
            uint4 kw[ABW_UNROLL], vw[ABW_UNROLL];
#pragma unroll
            for (u32 u = 0; u < ABW_UNROLL; ++u) {
                const u32 col = __shfl(cj, static_cast<int>((j + u) * G + g));
                kw[u] = liveK ? row_of(a.K, a.kBytes, col) : zero;
                vw[u] = liveV ? row_of(a.V, a.vBytes, col) : zero;
            }
#pragma unroll
            for (u32 u = 0; u < ABW_UNROLL; ++u) entry(kw[u], vw[u], true);
        }
        for (; j * G < nb; ++j) {  // the remaining steps; the last may be partly filled
            const u32 idx = j * G + g;
            const u32 col = __shfl(cj, static_cast<int>(idx & 63u));
            const bool valid = idx < nb;
            entry(liveK && valid ? row_of(a.K, a.kBytes, col) : zero, liveV && valid ? row_of(a.V, a.vBytes, col) : zero,
                  valid);
        }
        cj = next;
    }
    group_total<EPL>(acc, L, G, l);
    if (g == 0 && liveK) {
        float* o = sg.part == SPMM_DIRECT ? a.Y0 + row * a.D : a.P0 + static_cast<size_t>(sg.part) * a.D;
        store_f32<EPL>(o + static_cast<size_t>(l) * EPL, acc);
    }
}

template <int DT, int LANES>
__global__ __launch_bounds__(ABW_WAVES * 64) void k_attention_bwd_cols(const BwdArgs a) {
    using E = Elem<DT>;
    constexpr int EPL = E::EPL;
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 segId = blockIdx.x * ABW_WAVES + wave;
    if (segId >= a.nSegs) return;
    const SpmmSeg sg = a.segs[segId];
    const u32 L = LANES ? static_cast<u32>(LANES) : a.lanes;
    const u32 G = 64u / L;
    const u32 g = lane / L, l = lane % L;
    const bool liveK = l * 16u < a.kBytes, liveV = l * 16u < a.vBytes;
    const size_t colj = sg.dst;

    float k[EPL], v[EPL], accK[EPL], accV[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) k[i] = v[i] = accK[i] = accV[i] = 0.f;
    if (liveK) E::unpack(*reinterpret_cast<const uint4*>(a.K + colj * a.kBytes + l * 16u), k);
    if (liveV) E::unpack(*reinterpret_cast<const uint4*>(a.V + colj * a.vBytes + l * 16u), v);

    // a batch's rows with their LSE and delta, one entry per lane; the next batch's are loaded under
    // the current one's gathers
    auto batch = [&](u32 b0, u32& mi, float& ml, float& md) {
        mi = 0;
        ml = md = 0.f;
        if (b0 + lane < sg.count) {
            mi = a.idx[static_cast<size_t>(sg.first) + b0 + lane];
            ml = a.lse[mi];
            md = a.delta[mi];
        }
    };
    // an entry's gathered operands: the Q chunk as loaded, the lane's GO elements, the row's LSE and delta
    struct Ent {
        uint4 qw;
        float go[EPL];
        float lse, dl;
    };
    u32 mi, nmi = 0;
    float ml, md, nml = 0.f, nmd = 0.f;
    auto fetch = [&](u32 idx, bool valid) {
        Ent e;
        const int from = static_cast<int>(idx & 63u);
        const u32 r = __shfl(mi, from);
        e.lse = __shfl(ml, from);
        e.dl = __shfl(md, from);
        e.qw = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < EPL; ++i) e.go[i] = 0.f;
        if (valid) {
            if (liveK) e.qw = *reinterpret_cast<const uint4*>(a.Q + static_cast<size_t>(r) * a.kBytes + l * 16u);
            if (liveV) load_f32<EPL>(a.GO, r, a.Dv, l, e.go);
        }
        return e;
    };
    // every lane takes part in the shuffles; only the loads and the FMAs are predicated
    auto entry = [&](const Ent& e, bool valid) {
        float qx[EPL];
        E::unpack(e.qw, qx);
        const float p = group_dot<EPL>(qx, k, L);
        const float gg = group_dot<EPL>(e.go, v, L);
        float w, dp;
        weight_of(p, gg, e.lse, e.dl, a.scale, w, dp);
        if (valid) {
#pragma unroll
            for (int i = 0; i < EPL; ++i) {
                accK[i] = __builtin_fmaf(dp, qx[i], accK[i]);
                accV[i] = __builtin_fmaf(w, e.go[i], accV[i]);
            }
        }
    };
    batch(0, mi, ml, md);
    for (u32 b0 = 0; b0 < sg.count; b0 += 64u) {
        if (b0 + 64u < sg.count) batch(b0 + 64u, nmi, nml, nmd);
        const u32 nb = min(64u, sg.count - b0);
        const u32 full = nb / G;
        u32 j = 0;
        static_assert(ABW_UNROLL == 2, "two entries in flight, written out");
        for (; j + ABW_UNROLL <= full; j += ABW_UNROLL) {
            const Ent e0 = fetch(j * G + g, true);
            const Ent e1 = fetch((j + 1u) * G + g, true);
            entry(e0, true);
            entry(e1, true);
        }
        for (; j * G < nb; ++j) {
            const u32 idx = j * G + g;
            const bool valid = idx < nb;
            entry(fetch(idx, valid), valid);
        }
        mi = nmi;
        ml = nml;
        md = nmd;
    }
    group_total<EPL>(accK, L, G, l);
    group_total<EPL>(accV, L, G, l);
    if (g == 0) {
        const bool direct = sg.part == SPMM_DIRECT;
        if (liveK && a.Y0) {
            float* o = direct ? a.Y0 + colj * a.D : a.P0 + static_cast<size_t>(sg.part) * a.D;
            store_f32<EPL>(o + static_cast<size_t>(l) * EPL, accK);
        }
        if (liveV && a.Y1) {
            float* o = direct ? a.Y1 + colj * a.Dv : a.P1 + static_cast<size_t>(sg.part) * a.Dv;
            store_f32<EPL>(o + static_cast<size_t>(l) * EPL, accV);
        }
    }
}

// k_spmm_reduce for up to two outputs that share the split destinations: Y[dst] = the destination's
// partial rows added in segment order; one thread per four columns of Y0 (K0 columns, or none: Y0
// null) followed by Y1 (K1 columns, or none)
__global__ __launch_bounds__(256) void k_attention_bwd_reduce(const SpmmRed* reds, u32 nReds, const float* P0,
                                                              float* Y0, u32 K0, const float* P1, float* Y1, u32 K1) {
    const u32 q0 = Y0 ? K0 / 4u : 0u, q1 = Y1 ? K1 / 4u : 0u, q4 = q0 + q1;
    const size_t t = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= static_cast<size_t>(nReds) * q4) return;
    const SpmmRed r = reds[t / q4];
    u32 q = static_cast<u32>(t % q4);
    const bool second = q >= q0;
    if (second) q -= q0;
    const u32 K = second ? K1 : K0;
    const float* P = second ? P1 : P0;
    float* Y = second ? Y1 : Y0;
    const float4* p = reinterpret_cast<const float4*>(P + static_cast<size_t>(r.part0) * K) + q;
    float4 s = p[0];
    for (u32 i = 1; i < r.nparts; ++i) {
        const float4 x = p[static_cast<size_t>(i) * (K / 4u)];
        s.x += x.x;
        s.y += x.y;
        s.z += x.z;
        s.w += x.w;
    }
    reinterpret_cast<float4*>(Y + static_cast<size_t>(r.dst) * K)[q] = s;
}

using BwdFn = void (*)(const BwdArgs);

template <int DT>
BwdFn pick_rows(u32 rowBytes) {
    switch (rowBytes) {
        case 128: return k_attention_bwd_rows<DT, 8>;
        case 256: return k_attention_bwd_rows<DT, 16>;
        case 512: return k_attention_bwd_rows<DT, 32>;
        case 1024: return k_attention_bwd_rows<DT, 64>;
        default: return k_attention_bwd_rows<DT, 0>;
    }
}

template <int DT>
BwdFn pick_cols(u32 rowBytes) {
    switch (rowBytes) {
        case 128: return k_attention_bwd_cols<DT, 8>;
        case 256: return k_attention_bwd_cols<DT, 16>;
        case 512: return k_attention_bwd_cols<DT, 32>;
        case 1024: return k_attention_bwd_cols<DT, 64>;
        default: return k_attention_bwd_cols<DT, 0>;
    }
}

bool backward_ready(const Plan::AttentionBwdState& S, u32 D, u32 Dv) {
    return S.built && S.rowScratch.size() >= static_cast<size_t>(S.rowPartials) * D &&
           S.colScratch.size() >= static_cast<size_t>(S.colPartials) * (static_cast<size_t>(D) + Dv);
}

// build both sides' lists and delta (once) and size the scratches for (D, Dv); layout_mu held.
// Synchronous on the plan's stream.
int build_backward(const Plan& p, u32 D, u32 Dv) {
    const char* who = "bsmr_plan_prepare_attention_backward";
    Plan::AttentionBwdState& S = p.attention_bwd;
    const hipStream_t s = p.stream;
    if (!S.built) {
        SpmmLists R, C;
        const bool share = p.attention.built && attn_forward_chunk() == ATTN_BWD_ROW_CHUNK;
        if (!share) BSMR_CHECK(attn_row_lists(p, ATTN_BWD_ROW_CHUNK, who, R));
        {
            std::vector<u32> hrp, hci;
            BSMR_CHECK(p.rowptr.download(hrp, s));
            BSMR_CHECK(p.colidx.download(hci, s));
            SpmmIn in;
            in.M = p.M;
            in.N = p.N;
            in.nnz = p.nnz;
            in.rowptr = hrp.data();
            in.colidx = hci.data();
            in.side = 2;
            in.chunk = ATTN_BWD_COL_CHUNK;
            std::string err;
            if (spmm_lists(in, C, err)) {
                set_error(std::string(who) + ": " + err);
                return BSMR_ERR_INVALID;
            }
            if (C.nSegs > (1ull << 31)) {
                set_error(std::string(who) + ": more than 2^31 segments");
                return BSMR_ERR_UNSUPPORTED;
            }
        }
        if (!share) {
            BSMR_CHECK(S.rsegs.upload(R.segs.data(), R.segs.size(), s));
            BSMR_CHECK(S.rreds.upload(R.reds.data(), R.reds.size(), s));
        }
        BSMR_CHECK(S.csegs.upload(C.segs.data(), C.segs.size(), s));
        BSMR_CHECK(S.creds.upload(C.reds.data(), C.reds.size(), s));
        BSMR_CHECK(S.csrc.upload(C.src.data(), C.src.size(), s));
        BSMR_CHECK(S.delta.alloc(p.M));
        BSMR_HIP(hipStreamSynchronize(s));
        S.rowShared = share;
        if (share) {
            const Plan::AttentionState& F = p.attention;
            S.rowSegs = F.nSegs;
            S.rowReds = F.nReds;
            S.rowSplit = F.splitRows;
            S.rowPartials = F.partials;
            S.rowMax = F.maxRow;
        } else {
            S.rowSegs = static_cast<u32>(R.nSegs);
            S.rowReds = static_cast<u32>(R.reds.size());
            S.rowSplit = R.splitDsts;
            S.rowPartials = R.partials;
            S.rowMax = R.maxList;
        }
        S.colSegs = static_cast<u32>(C.nSegs);
        S.colReds = static_cast<u32>(C.reds.size());
        S.colSplit = C.splitDsts;
        S.colPartials = C.partials;
        S.colMax = C.maxList;
        S.built = true;
    }
    const size_t rowNeed = static_cast<size_t>(S.rowPartials) * D;
    const size_t colNeed = static_cast<size_t>(S.colPartials) * (static_cast<size_t>(D) + Dv);
    if (S.rowScratch.size() < rowNeed) BSMR_CHECK(S.rowScratch.alloc(rowNeed));
    if (S.colScratch.size() < colNeed) BSMR_CHECK(S.colScratch.alloc(colNeed));
    return BSMR_OK;
}

}  // namespace
}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_attention_backward(const bsmr_plan* plan, const void* dQ, const void* dK, const void* dV,
                                       const float* dO, const float* dGO, const float* dLse, uint32_t D, uint32_t Dv,
                                       int dtype, float scale, float* dGQ, float* dGK, float* dGV, void* stream) {
    const char* who = "bsmr_attention_backward";
    if (!plan) {
        set_error("bsmr_attention_backward: null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dQ || !dK || !dV || !dO || !dGO || !dLse) {
        set_error("bsmr_attention_backward: null device pointer");
        return BSMR_ERR_INVALID;
    }
    if (!dGQ && !dGK && !dGV) {
        set_error("bsmr_attention_backward: dGQ, dGK and dGV are all null: nothing to compute");
        return BSMR_ERR_INVALID;
    }
    if (!attn_aligned16(dQ) || !attn_aligned16(dK) || !attn_aligned16(dV) || !attn_aligned16(dO) ||
        !attn_aligned16(dGO) || !attn_aligned16(dGQ) || !attn_aligned16(dGK) || !attn_aligned16(dGV) ||
        (reinterpret_cast<uintptr_t>(dLse) & 3u)) {
        set_error("bsmr_attention_backward: dQ, dK, dV, dO, dGO, dGQ, dGK and dGV must be 16-byte aligned");
        return BSMR_ERR_INVALID;
    }
    float c;
    BSMR_CHECK(attn_validate_scale(who, scale, &c));
    BSMR_CHECK(attn_validate_dims(who, D, Dv, dtype));
    const Plan& p = plan->p;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Plan::AttentionBwdState& S = p.attention_bwd;
    BwdArgs r{}, cs{};
    const SpmmRed *rreds = nullptr, *creds = nullptr;
    u32 rowReds = 0, colReds = 0, colPartials = 0;
    float* colScratch = nullptr;
    {
        std::lock_guard<std::mutex> g(p.layout_mu);
        if (!backward_ready(S, D, Dv)) {
            const LaunchSite at{s, who, "bsmr_plan_prepare_attention_backward", D, dtype};
            const int st = lazy_build_guard(at);
            if (st == BSMR_ERR_NOT_PREPARED)  // (the guard's own message names a (K, dtype) layout)
                set_error("bsmr_attention_backward: stream is capturing and the backward lists (or their scratch for D = " +
                          std::to_string(D) + ", Dv = " + std::to_string(Dv) +
                          ") are not built; call bsmr_plan_prepare_attention_backward first");
            BSMR_CHECK(st);
            BSMR_CHECK(build_backward(p, D, Dv));
        }
        r.segs = S.row_segs(p.attention);
        r.nSegs = S.rowSegs;
        r.P0 = S.rowScratch.data();
        r.delta = S.delta.data();
        rreds = S.row_reds(p.attention);
        rowReds = S.rowReds;
        cs.segs = S.csegs.data();
        cs.nSegs = S.colSegs;
        cs.idx = S.csrc.data();
        creds = S.creds.data();
        colReds = S.colReds;
        colPartials = S.colPartials;
        colScratch = S.colScratch.data();
    }
    const u32 esz = dtype == BSMR_F32 ? 4u : 2u;
    r.idx = p.colidx.data();
    r.Q = cs.Q = static_cast<const char*>(dQ);
    r.K = cs.K = static_cast<const char*>(dK);
    r.V = cs.V = static_cast<const char*>(dV);
    r.GO = cs.GO = dGO;
    r.lse = cs.lse = dLse;
    cs.delta = r.delta;
    r.D = cs.D = D;
    r.Dv = cs.Dv = Dv;
    r.kBytes = cs.kBytes = D * esz;
    r.vBytes = cs.vBytes = Dv * esz;
    r.scale = cs.scale = scale;
    const u32 rowBytes = std::max(r.kBytes, r.vBytes);
    r.lanes = cs.lanes = attn_lanes(rowBytes);
    r.Y0 = dGQ;
    cs.Y0 = dGK;
    cs.Y1 = dGV;
    cs.P0 = colScratch;
    cs.P1 = colScratch ? colScratch + static_cast<size_t>(colPartials) * D : nullptr;

    if (p.M) {
        const u32 epl = 16u / esz, perBlock = 4u * (64u / r.lanes);
        const u32 grid = static_cast<u32>((static_cast<size_t>(p.M) + perBlock - 1) / perBlock);
        float* delta = const_cast<float*>(r.delta);
        if (epl == 4)
            hipLaunchKernelGGL(k_attention_bwd_delta<4>, dim3(grid), dim3(256), 0, s, dGO, dO, delta, p.M, Dv, r.lanes);
        else
            hipLaunchKernelGGL(k_attention_bwd_delta<8>, dim3(grid), dim3(256), 0, s, dGO, dO, delta, p.M, Dv, r.lanes);
        BSMR_HIP(hipGetLastError());
    }
    if (dGQ) {
        const BwdFn fn = dtype == BSMR_F32   ? pick_rows<BSMR_F32>(rowBytes)
                         : dtype == BSMR_F16 ? pick_rows<BSMR_F16>(rowBytes)
                                             : pick_rows<BSMR_BF16>(rowBytes);
        if (r.nSegs) {
            hipLaunchKernelGGL(fn, dim3((r.nSegs + ABW_WAVES - 1) / ABW_WAVES), dim3(ABW_WAVES * 64), 0, s, r);
            BSMR_HIP(hipGetLastError());
        }
        if (rowReds) {
            const size_t threads = static_cast<size_t>(rowReds) * (D / 4u);
            hipLaunchKernelGGL(k_attention_bwd_reduce, dim3(static_cast<u32>((threads + 255) / 256)), dim3(256), 0, s, rreds,
                               rowReds, r.P0, dGQ, D, static_cast<const float*>(nullptr), static_cast<float*>(nullptr), 0u);
            BSMR_HIP(hipGetLastError());
        }
    }
    if (dGK || dGV) {
        const BwdFn fn = dtype == BSMR_F32   ? pick_cols<BSMR_F32>(rowBytes)
                         : dtype == BSMR_F16 ? pick_cols<BSMR_F16>(rowBytes)
                                             : pick_cols<BSMR_BF16>(rowBytes);
        if (cs.nSegs) {
            hipLaunchKernelGGL(fn, dim3((cs.nSegs + ABW_WAVES - 1) / ABW_WAVES), dim3(ABW_WAVES * 64), 0, s, cs);
            BSMR_HIP(hipGetLastError());
        }
        if (colReds) {
            const size_t threads = static_cast<size_t>(colReds) * ((dGK ? D / 4u : 0u) + (dGV ? Dv / 4u : 0u));
            hipLaunchKernelGGL(k_attention_bwd_reduce, dim3(static_cast<u32>((threads + 255) / 256)), dim3(256), 0, s, creds,
                               colReds, cs.P0, dGK, D, cs.P1, dGV, Dv);
            BSMR_HIP(hipGetLastError());
        }
    }
    return BSMR_OK;
}

extern "C" int bsmr_plan_prepare_attention_backward(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    if (!plan) {
        set_error("bsmr_plan_prepare_attention_backward: null plan");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(attn_validate_prepare_dims("bsmr_plan_prepare_attention_backward", D, Dv));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_backward(plan->p, D, Dv);
}

extern "C" int bsmr_plan_attention_backward_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    if (!plan) {
        set_error("bsmr_plan_attention_backward_prepared: null plan");
        return 0;
    }
    if (attn_validate_prepare_dims("bsmr_plan_attention_backward_prepared", D, Dv) != BSMR_OK) return 0;
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return backward_ready(plan->p.attention_bwd, D, Dv) ? 1 : 0;
}

extern "C" int bsmr_plan_attention_backward_stats(const bsmr_plan* plan, bsmr_attention_backward_stats* out) {
    if (!plan || !out) {
        set_error("bsmr_plan_attention_backward_stats: null argument");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    const Plan::AttentionBwdState& S = p.attention_bwd;
    *out = bsmr_attention_backward_stats{};
    out->row_chunk = ATTN_BWD_ROW_CHUNK;
    out->col_chunk = ATTN_BWD_COL_CHUNK;
    if (S.built) {
        out->row_segments = S.rowSegs;
        out->row_split = S.rowSplit;
        out->row_partials = S.rowPartials;
        out->row_max = S.rowMax;
        out->col_segments = S.colSegs;
        out->col_split = S.colSplit;
        out->col_partials = S.colPartials;
        out->col_max = S.colMax;
        out->row_scratch_bytes = S.rowScratch.size() * sizeof(float);
        out->col_scratch_bytes = S.colScratch.size() * sizeof(float);
        out->delta_bytes = S.delta.size() * sizeof(float);
    }
    return BSMR_OK;
}

extern "C" void bsmr_attention_backward_limits(uint32_t* row_chunk, uint32_t* col_chunk, uint32_t* max_row_bytes) {
    if (row_chunk) *row_chunk = ATTN_BWD_ROW_CHUNK;
    if (col_chunk) *col_chunk = ATTN_BWD_COL_CHUNK;
    if (max_row_bytes) *max_row_bytes = ATTN_MAX_ROW_BYTES;
}
