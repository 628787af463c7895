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
//
// Batch and heads (bsmr_attention_backward_heads): the same kernels over Z = batches x heads slices
// in one grid, as in attention.hip: blockIdx.x the segment (or row group, or reduce thread block),
// blockIdx.y the head, blockIdx.z the batch; per-operand batch / head strides (64-bit, bytes) and
// row strides (32-bit, bytes); slice bases wave-uniform, computed once at kernel entry; LSE and
// delta dense (slices x M); scratch per slice. bsmr_attention_backward is the one-slice,
// dense-stride case of the same launch code.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "attention_common.hpp"
#include "attention_layout.hpp"
#include "plan.hpp"
#include "row_elems.hpp"
#include "seg_walk.hpp"
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
    AttnOpBytes Q;       // per slice M rows of kBytes
    AttnOpBytes K;       // per slice N rows of kBytes
    AttnOpBytes V;       // per slice N rows of vBytes
    AttnOpBytes GO;      // per slice M rows of Dv floats
    const float* lse;    // slices x M
    const float* delta;  // slices x M
    AttnOpBytes Y0;      // rows side: GQ (rows of D floats); columns side: GK (rows of D floats) or null
    AttnOpBytes Y1;      // columns side: GV (rows of Dv floats) or null
    float* P0;           // per slice: partial slots x D
    float* P1;           // columns side, per slice: partial slots x Dv
    u64 sliceScratch;    // floats of scratch per slice (both of P0 and P1)
    u32 heads, slices, M;  // slices = batches x heads
    u32 nSegs, D, Dv, kBytes, vBytes;
    u32 lanes;           // generic form: lanes per lane group (a power of two, 4 .. 64)
    float scale;
};

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

// the lane groups in group order (group g held entries g, g + G, ... of the segment): every lane
// ends with the same totals. (The forward's inline form of this lacks the unroll pragma below and
// stays apart: it keeps a 64-VGPR cap, and was neither built nor measured with it.)
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
struct DeltaArgs {
    AttnOpBytes GO;  // per slice M rows of Dv floats
    AttnOpBytes O;   // the same
    float* delta;    // slices x M
    u32 heads, slices, M, Dv, L;
};

template <int EPL>
__global__ __launch_bounds__(256) void k_attention_bwd_delta(const DeltaArgs a) {
    const char *GO = a.GO.ptr, *O = a.O.ptr;
    float* delta = a.delta;
    if (a.slices > 1u) {  // (one slice branches around the base arithmetic, as in the kernels below)
        const u32 head = blockIdx.y, bat = blockIdx.z;
        GO = attn_slice_base(a.GO, bat, head);
        O = attn_slice_base(a.O, bat, head);
        delta += (static_cast<size_t>(bat) * a.heads + head) * a.M;
    }
    const u32 M = a.M, Dv = a.Dv;
    const LaneGroups lg(a.L, threadIdx.x & 63u);
    const u32 L = lg.L, l = lg.l;
    const size_t row = (static_cast<size_t>(blockIdx.x) * 4u + (threadIdx.x >> 6)) * lg.G + lg.g;
    const bool live = row < M && l * static_cast<u32>(EPL) < Dv;
    float x[EPL], y[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) x[i] = y[i] = 0.f;
    if (live) {
        load_f32<EPL>(GO + row * a.GO.row, l, x);
        load_f32<EPL>(O + row * a.O.row, l, y);
    }
    const float d = group_dot<EPL>(x, y, L);
    if (row < M && l == 0) delta[row] = d;
}

// what the segment kernels and the reduce start from: the slice (head blockIdx.y of batch
// blockIdx.z) and its operands' bases, wave-uniform and 64-bit, in scalar registers. A call of one
// slice (bsmr_attention_backward) branches around the arithmetic and its argument loads
struct BwdSlice {
    size_t slice = 0;
    const char *Q, *K, *V, *GO;
    char *Y0, *Y1;
    __device__ __forceinline__ explicit BwdSlice(const BwdArgs& a)
        : Q(a.Q.ptr), K(a.K.ptr), V(a.V.ptr), GO(a.GO.ptr), Y0(a.Y0.ptr), Y1(a.Y1.ptr) {
        if (a.slices > 1u) {
            const u32 head = blockIdx.y, bat = blockIdx.z;
            slice = static_cast<size_t>(bat) * a.heads + head;
            Q = attn_slice_base(a.Q, bat, head);
            K = attn_slice_base(a.K, bat, head);
            V = attn_slice_base(a.V, bat, head);
            GO = attn_slice_base(a.GO, bat, head);
            Y0 = attn_slice_base(a.Y0, bat, head);
            Y1 = attn_slice_base(a.Y1, bat, head);
        }
    }
};

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
    const BwdSlice s(a);
    const LaneGroups lg(LANES ? static_cast<u32>(LANES) : a.lanes, lane);
    const u32 L = lg.L, G = lg.G, g = lg.g, l = lg.l;
    const bool liveK = l * 16u < a.kBytes, liveV = l * 16u < a.vBytes;
    const size_t row = sg.dst;

    float q[EPL], go[EPL], acc[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) q[i] = go[i] = acc[i] = 0.f;
    if (liveK) E::unpack(*reinterpret_cast<const uint4*>(s.Q + row * a.Q.row + l * 16u), q);
    if (liveV) load_f32<EPL>(s.GO + row * a.GO.row, l, go);
    const float lse = a.lse[s.slice * a.M + row], dl = a.delta[s.slice * a.M + row];

    // an entry's K and V chunks as loaded (zeros for a lane past the row or an idle tail entry; a
    // zero by name in `cond ? *ptr : zero` would be selected by address, from scratch)
    struct Ent {
        uint4 kw, vw;
    };
    auto batch = [&](u32 b0) {
        return b0 + lane < sg.count ? a.idx[static_cast<size_t>(sg.first) + b0 + lane] : 0u;
    };
    auto row_of = [&](const char* X, u32 rowBytes, size_t col) {
        return *reinterpret_cast<const uint4*>(X + col * rowBytes + l * 16u);
    };
    auto fetch = [&](u32 cj, u32 idx, bool valid, Ent& e) {
        const u32 col = __shfl(cj, static_cast<int>(idx & 63u));
        e.kw = liveK && valid ? row_of(s.K, a.K.row, col) : make_uint4(0, 0, 0, 0);
        e.vw = liveV && valid ? row_of(s.V, a.V.row, col) : make_uint4(0, 0, 0, 0);
    };
    // every lane takes part in the shuffles; only the loads and the FMAs into acc are predicated
    auto use = [&](const Ent& e, u32, bool valid) {
        float kx[EPL], vx[EPL];
        E::unpack(e.kw, kx);
        E::unpack(e.vw, vx);
        const float p = group_dot<EPL>(q, kx, L);
        const float gg = group_dot<EPL>(go, vx, L);
        float w, dp;
        weight_of(p, gg, lse, dl, a.scale, w, dp);
        if (valid) {
#pragma unroll
            for (int i = 0; i < EPL; ++i) acc[i] = __builtin_fmaf(dp, kx[i], acc[i]);
        }
    };
    seg_walk<ABW_UNROLL, Ent>(sg.count, G, g, batch(0), batch, fetch, use);
    group_total<EPL>(acc, L, G, l);
    if (g == 0 && liveK) {
        float* o = sg.part == SPMM_DIRECT
                       ? reinterpret_cast<float*>(s.Y0 + row * a.Y0.row)
                       : a.P0 + s.slice * a.sliceScratch + static_cast<size_t>(sg.part) * a.D;
        store_f32<EPL>(o + static_cast<size_t>(l) * EPL, acc);
    }
}

// The columns side keeps its hand-written copy of the loop that the rows side takes from seg_walk:
// on the walker it measured 1.1 % slower at fp32 D = 64 on C3
template <int DT, int LANES>
__global__ __launch_bounds__(ABW_WAVES * 64) void k_attention_bwd_cols(const BwdArgs a) {
    using E = Elem<DT>;
    constexpr int EPL = E::EPL;
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 segId = blockIdx.x * ABW_WAVES + wave;
    if (segId >= a.nSegs) return;
    const SpmmSeg sg = a.segs[segId];
    const BwdSlice s(a);
    const size_t slice = s.slice;
    const char *Qs = s.Q, *Ks = s.K, *Vs = s.V, *GOs = s.GO;
    char *Y0s = s.Y0, *Y1s = s.Y1;
    const float* const lses = a.lse + slice * a.M;
    const float* const deltas = a.delta + slice * a.M;
    const LaneGroups lg(LANES ? static_cast<u32>(LANES) : a.lanes, lane);
    const u32 L = lg.L, G = lg.G, g = lg.g, l = lg.l;
    const bool liveK = l * 16u < a.kBytes, liveV = l * 16u < a.vBytes;
    const size_t colj = sg.dst;

    float k[EPL], v[EPL], accK[EPL], accV[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) k[i] = v[i] = accK[i] = accV[i] = 0.f;
    if (liveK) E::unpack(*reinterpret_cast<const uint4*>(Ks + colj * a.K.row + l * 16u), k);
    if (liveV) E::unpack(*reinterpret_cast<const uint4*>(Vs + colj * a.V.row + l * 16u), v);

    // a batch's rows with their LSE and delta, one entry per lane; the next batch's are loaded under
    // the current one's gathers
    auto batch = [&](u32 b0, u32& mi, float& ml, float& md) {
        mi = 0;
        ml = md = 0.f;
        if (b0 + lane < sg.count) {
            mi = a.idx[static_cast<size_t>(sg.first) + b0 + lane];
            ml = lses[mi];
            md = deltas[mi];
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
            if (liveK) e.qw = *reinterpret_cast<const uint4*>(Qs + static_cast<size_t>(r) * a.Q.row + l * 16u);
            if (liveV) load_f32<EPL>(GOs + static_cast<size_t>(r) * a.GO.row, l, e.go);
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
        if (liveK && a.Y0.ptr) {
            float* o = direct ? reinterpret_cast<float*>(Y0s + colj * a.Y0.row)
                              : a.P0 + slice * a.sliceScratch + static_cast<size_t>(sg.part) * a.D;
            store_f32<EPL>(o + static_cast<size_t>(l) * EPL, accK);
        }
        if (liveV && a.Y1.ptr) {
            float* o = direct ? reinterpret_cast<float*>(Y1s + colj * a.Y1.row)
                              : a.P1 + slice * a.sliceScratch + static_cast<size_t>(sg.part) * a.Dv;
            store_f32<EPL>(o + static_cast<size_t>(l) * EPL, accV);
        }
    }
}

// k_spmm_reduce for up to two outputs that share the split destinations: Y[dst] = the destination's
// partial rows added in segment order; one thread per four columns of Y0 (K0 columns, or none: Y0
// null) followed by Y1 (K1 columns, or none)
__global__ __launch_bounds__(256) void k_attention_bwd_reduce(const BwdArgs a, const SpmmRed* reds, u32 nReds) {
    const BwdSlice sl(a);
    const size_t sliceOff = sl.slice * a.sliceScratch;
    const u32 K0 = a.D, K1 = a.Dv;
    const u32 q0 = a.Y0.ptr ? K0 / 4u : 0u, q1 = a.Y1.ptr ? K1 / 4u : 0u, q4 = q0 + q1;
    const size_t t = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= static_cast<size_t>(nReds) * q4) return;
    const SpmmRed r = reds[t / q4];
    u32 q = static_cast<u32>(t % q4);
    const bool second = q >= q0;
    if (second) q -= q0;
    const u32 K = second ? K1 : K0;
    const float* P = (second ? a.P1 : a.P0) + sliceOff;
    char* Y = second ? sl.Y1 + static_cast<size_t>(r.dst) * a.Y1.row : sl.Y0 + static_cast<size_t>(r.dst) * a.Y0.row;
    const float4* p = reinterpret_cast<const float4*>(P + static_cast<size_t>(r.part0) * K) + q;
    float4 s = p[0];
    for (u32 i = 1; i < r.nparts; ++i) {
        const float4 x = p[static_cast<size_t>(i) * (K / 4u)];
        s.x += x.x;
        s.y += x.y;
        s.z += x.z;
        s.w += x.w;
    }
    reinterpret_cast<float4*>(Y)[q] = s;
}

using BwdFn = void (*)(const BwdArgs);

// the segment kernel of a side (rows or columns) for rows of rowBytes: the fixed sizes or the generic form
template <int DT>
BwdFn pick_side(bool rows, u32 rowBytes) {
    switch (rowBytes) {
        case 128: return rows ? k_attention_bwd_rows<DT, 8> : k_attention_bwd_cols<DT, 8>;
        case 256: return rows ? k_attention_bwd_rows<DT, 16> : k_attention_bwd_cols<DT, 16>;
        case 512: return rows ? k_attention_bwd_rows<DT, 32> : k_attention_bwd_cols<DT, 32>;
        case 1024: return rows ? k_attention_bwd_rows<DT, 64> : k_attention_bwd_cols<DT, 64>;
        default: return rows ? k_attention_bwd_rows<DT, 0> : k_attention_bwd_cols<DT, 0>;
    }
}

BwdFn pick_side(int dtype, bool rows, u32 rowBytes) {
    return dtype == BSMR_F32   ? pick_side<BSMR_F32>(rows, rowBytes)
           : dtype == BSMR_F16 ? pick_side<BSMR_F16>(rows, rowBytes)
                               : pick_side<BSMR_BF16>(rows, rowBytes);
}

bool backward_ready(const Plan& p, u32 D, u32 Dv, u32 slices) {
    const Plan::AttentionBwdState& S = p.attention_bwd;
    // (DevBuf holds a size only with its memory: a failed grow leaves the old buffer and its size)
    return S.built && S.delta.size() >= attn_sat_mul(slices, p.M) &&
           S.rowScratch.size() >= attn_sat_mul(slices, S.rowPartials, D) &&
           S.colScratch.size() >= attn_sat_mul(slices, S.colPartials, static_cast<size_t>(D) + Dv);
}

// build both sides' lists (once) and size delta and the per-slice scratches for (D, Dv, slices):
// they grow and never shrink; layout_mu held. Synchronous on the plan's stream.
int build_backward(const Plan& p, u32 D, u32 Dv, u32 slices, const char* who) {
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
    BSMR_CHECK(S.delta.grow(attn_sat_mul(slices, p.M)));
    BSMR_CHECK(S.rowScratch.grow(attn_sat_mul(slices, S.rowPartials, D)));
    BSMR_CHECK(S.colScratch.grow(attn_sat_mul(slices, S.colPartials, static_cast<size_t>(D) + Dv)));
    return BSMR_OK;
}

struct BwdOperands {
    const bsmr_attention_operand *Q, *K, *V, *O, *GO, *GQ, *GK, *GV;  // the last three may be null, not all
};

// the launches of bsmr_attention_backward and bsmr_attention_backward_heads, arguments already
// validated: `who` and `prep` name the entry point and its prepare call in errors
int backward_launch(const char* who, const char* prep, const bsmr_plan* plan, u32 batches, u32 heads,
                    const BwdOperands& x, const float* dLse, u32 D, u32 Dv, int dtype, float scale, void* stream) {
    const Plan& p = plan->p;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Plan::AttentionBwdState& S = p.attention_bwd;
    const u32 slices = batches * heads;  // (both at most 65535)
    BwdArgs r{}, cs{};
    const SpmmRed *rreds = nullptr, *creds = nullptr;
    u32 rowReds = 0, colReds = 0, rowPartials = 0, colPartials = 0;
    float* colScratch = nullptr;
    {
        std::lock_guard<std::mutex> g(p.layout_mu);
        if (!backward_ready(p, D, Dv, slices)) {
            const LaunchSite at{s, who, prep, D, dtype};
            const int st = lazy_build_guard(at);
            if (st == BSMR_ERR_NOT_PREPARED)  // (the guard's own message names a (K, dtype) layout)
                set_error(std::string(who) + ": stream is capturing and the backward lists (or their scratch for D = " +
                          std::to_string(D) + ", Dv = " + std::to_string(Dv) +
                          (slices > 1 ? ", " + std::to_string(slices) + " slices" : std::string()) +
                          ") are not built; call " + prep + " first");
            BSMR_CHECK(st);
            BSMR_CHECK(build_backward(p, D, Dv, slices, prep));
        }
        r.segs = S.row_segs(p.attention);
        r.nSegs = S.rowSegs;
        r.P0 = S.rowScratch.data();
        r.delta = S.delta.data();
        rreds = S.row_reds(p.attention);
        rowReds = S.rowReds;
        rowPartials = S.rowPartials;
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
    r.Q = cs.Q = attn_op_bytes(x.Q, batches, heads, p.M, esz);
    r.K = cs.K = attn_op_bytes(x.K, batches, heads, p.N, esz);
    r.V = cs.V = attn_op_bytes(x.V, batches, heads, p.N, esz);
    r.GO = cs.GO = attn_op_bytes(x.GO, batches, heads, p.M, 4u);
    r.lse = cs.lse = dLse;
    cs.delta = r.delta;
    r.heads = cs.heads = heads;
    r.slices = cs.slices = slices;
    r.M = cs.M = p.M;
    r.D = cs.D = D;
    r.Dv = cs.Dv = Dv;
    r.kBytes = cs.kBytes = D * esz;
    r.vBytes = cs.vBytes = Dv * esz;
    r.scale = cs.scale = scale;
    const u32 rowBytes = std::max(r.kBytes, r.vBytes);
    r.lanes = cs.lanes = attn_lanes(rowBytes);
    r.Y0 = attn_op_bytes(x.GQ, batches, heads, p.M, 4u);
    r.sliceScratch = static_cast<u64>(rowPartials) * D;
    cs.Y0 = attn_op_bytes(x.GK, batches, heads, p.N, 4u);
    cs.Y1 = attn_op_bytes(x.GV, batches, heads, p.N, 4u);
    cs.P0 = colScratch;
    cs.P1 = colScratch ? colScratch + static_cast<size_t>(colPartials) * D : nullptr;
    cs.sliceScratch = static_cast<u64>(colPartials) * (static_cast<u64>(D) + Dv);

    if (p.M) {
        const u32 epl = 16u / esz, perBlock = 4u * (64u / r.lanes);
        const u32 grid = static_cast<u32>((static_cast<size_t>(p.M) + perBlock - 1) / perBlock);
        DeltaArgs d{};
        d.GO = r.GO;
        d.O = attn_op_bytes(x.O, batches, heads, p.M, 4u);
        d.delta = const_cast<float*>(r.delta);
        d.heads = heads;
        d.slices = slices;
        d.M = p.M;
        d.Dv = Dv;
        d.L = r.lanes;
        if (epl == 4)
            hipLaunchKernelGGL(k_attention_bwd_delta<4>, dim3(grid, heads, batches), dim3(256), 0, s, d);
        else
            hipLaunchKernelGGL(k_attention_bwd_delta<8>, dim3(grid, heads, batches), dim3(256), 0, s, d);
        BSMR_HIP(hipGetLastError());
    }
    if (x.GQ) {
        const BwdFn fn = pick_side(dtype, true, rowBytes);
        if (r.nSegs) {
            hipLaunchKernelGGL(fn, dim3((r.nSegs + ABW_WAVES - 1) / ABW_WAVES, heads, batches), dim3(ABW_WAVES * 64), 0, s,
                               r);
            BSMR_HIP(hipGetLastError());
        }
        if (rowReds) {
            const size_t threads = static_cast<size_t>(rowReds) * (D / 4u);
            hipLaunchKernelGGL(k_attention_bwd_reduce, dim3(static_cast<u32>((threads + 255) / 256), heads, batches),
                               dim3(256), 0, s, r, rreds, rowReds);
            BSMR_HIP(hipGetLastError());
        }
    }
    if (x.GK || x.GV) {
        const BwdFn fn = pick_side(dtype, false, rowBytes);
        if (cs.nSegs) {
            hipLaunchKernelGGL(fn, dim3((cs.nSegs + ABW_WAVES - 1) / ABW_WAVES, heads, batches), dim3(ABW_WAVES * 64), 0, s,
                               cs);
            BSMR_HIP(hipGetLastError());
        }
        if (colReds) {
            const size_t threads = static_cast<size_t>(colReds) * ((x.GK ? D / 4u : 0u) + (x.GV ? Dv / 4u : 0u));
            hipLaunchKernelGGL(k_attention_bwd_reduce, dim3(static_cast<u32>((threads + 255) / 256), heads, batches),
                               dim3(256), 0, s, cs, creds, colReds);
            BSMR_HIP(hipGetLastError());
        }
    }
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
    const bsmr_attention_operand q = attention_dense_operand(dQ, 1, p.M, D), k = attention_dense_operand(dK, 1, p.N, D),
                                 v = attention_dense_operand(dV, 1, p.N, Dv), o = attention_dense_operand(dO, 1, p.M, Dv),
                                 go = attention_dense_operand(dGO, 1, p.M, Dv), gq = attention_dense_operand(dGQ, 1, p.M, D),
                                 gk = attention_dense_operand(dGK, 1, p.N, D), gv = attention_dense_operand(dGV, 1, p.N, Dv);
    const BwdOperands x{&q, &k, &v, &o, &go, dGQ ? &gq : nullptr, dGK ? &gk : nullptr, dGV ? &gv : nullptr};
    return backward_launch(who, "bsmr_plan_prepare_attention_backward", plan, 1, 1, x, dLse, D, Dv, dtype, scale, stream);
}

extern "C" int bsmr_attention_backward_heads(const bsmr_plan* plan, uint32_t batches, uint32_t heads,
                                             const bsmr_attention_operand* Q, const bsmr_attention_operand* K,
                                             const bsmr_attention_operand* V, const bsmr_attention_operand* O,
                                             const bsmr_attention_operand* GO, const float* dLse, uint32_t D, uint32_t Dv,
                                             int dtype, float scale, const bsmr_attention_operand* GQ,
                                             const bsmr_attention_operand* GK, const bsmr_attention_operand* GV,
                                             void* stream) {
    const char* who = "bsmr_attention_backward_heads";
    if (!plan) {
        set_error("bsmr_attention_backward_heads: null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dLse || (reinterpret_cast<uintptr_t>(dLse) & 3u)) {
        set_error("bsmr_attention_backward_heads: dLse must be non-null and 4-byte aligned");
        return BSMR_ERR_INVALID;
    }
    if (!GQ && !GK && !GV) {
        set_error("bsmr_attention_backward_heads: GQ, GK and GV are all null: nothing to compute");
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
    BSMR_CHECK(attn_check_operand(who, "O", O, batches, heads, p.M, Dv, 4u, false));
    BSMR_CHECK(attn_check_operand(who, "GO", GO, batches, heads, p.M, Dv, 4u, false));
    if (GQ) BSMR_CHECK(attn_check_operand(who, "GQ", GQ, batches, heads, p.M, D, 4u, true));
    if (GK) BSMR_CHECK(attn_check_operand(who, "GK", GK, batches, heads, p.N, D, 4u, true));
    if (GV) BSMR_CHECK(attn_check_operand(who, "GV", GV, batches, heads, p.N, Dv, 4u, true));
    const BwdOperands x{Q, K, V, O, GO, GQ, GK, GV};
    return backward_launch(who, "bsmr_plan_prepare_attention_backward_heads", plan, batches, heads, x, dLse, D, Dv, dtype,
                           scale, stream);
}

extern "C" int bsmr_plan_prepare_attention_backward(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    if (!plan) {
        set_error("bsmr_plan_prepare_attention_backward: null plan");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(attn_validate_prepare_dims("bsmr_plan_prepare_attention_backward", D, Dv));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_backward(plan->p, D, Dv, 1, "bsmr_plan_prepare_attention_backward");
}

extern "C" int bsmr_plan_attention_backward_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    if (!plan) {
        set_error("bsmr_plan_attention_backward_prepared: null plan");
        return 0;
    }
    if (attn_validate_prepare_dims("bsmr_plan_attention_backward_prepared", D, Dv) != BSMR_OK) return 0;
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return backward_ready(plan->p, D, Dv, 1) ? 1 : 0;
}

extern "C" int bsmr_plan_prepare_attention_backward_heads(const bsmr_plan* plan, uint32_t D, uint32_t Dv,
                                                          uint32_t slices) {
    const char* who = "bsmr_plan_prepare_attention_backward_heads";
    if (!plan) {
        set_error("bsmr_plan_prepare_attention_backward_heads: null plan");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(attn_check_slices(who, slices));
    BSMR_CHECK(attn_validate_prepare_dims(who, D, Dv));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_backward(plan->p, D, Dv, slices, who);
}

extern "C" int bsmr_plan_attention_backward_heads_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv,
                                                           uint32_t slices) {
    const char* who = "bsmr_plan_attention_backward_heads_prepared";
    if (!plan) {
        set_error("bsmr_plan_attention_backward_heads_prepared: null plan");
        return 0;
    }
    if (attn_check_slices(who, slices) != BSMR_OK || attn_validate_prepare_dims(who, D, Dv) != BSMR_OK) return 0;
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return backward_ready(plan->p, D, Dv, slices) ? 1 : 0;
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
