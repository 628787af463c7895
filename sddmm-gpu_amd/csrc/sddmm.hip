// sddmm.hip — the SDDMM entry points over a BSMR plan (gfx950, wave64, MFMA) and the launches they
// choose between (launch_select.cpp choose_launch):
//   * the column-major fp32 launch (launch_full, k_sddmm_f32) and its panel-range form
//     (launch_panels, k_sddmm_panels_f32): the kernels are in this file, described below;
//   * the row-block launch (launch_rb, every dtype): its layout cache (get_rb_layout) and argument
//     set-up are here, the kernels k_sddmm_rb / k_sddmm_rb_pair and pick_rb in rb_kernel.hpp, which
//     this file includes, so they are part of this translation unit;
//   * the column-major fp16 / bf16, panel-tile and dense-sampled launches: sddmm_half.hip and
//     sddmm_dense.hip, called from here.
// Then bsmr_sddmm / _batch / _panels / _panels_local, bsmr_plan_prepare*, bsmr_sddmm_profile and
// the debug exports (bsmr_debug_*, not in the header).
//
// The column-major launch: one wave per work item (256-thread workgroups of four independent
// waves; 64-thread workgroups for panel ranges), two item kinds:
//   * dense tile {panel, tile}: 4*K/16 `v_mfma_f32_16x16x4_f32` (exact fp32; gfx950 has no TF32).
//     Lane l holds A[row l&15][16kk + 4(l>>4) + e] and B[col l&15][same k]; instruction e of step
//     kk sums k = 16kk + 4g + e over the four lane groups g, so every k is covered once.
//     Accumulator lane l, reg r = D[4(l>>4)+r][l&15], scattered through blockValues
//     (replaces sddmm_gpu_dense_block_m16n16k8_*, sddmmKernel.cu:213-351, 355-488).
//   * residual slot {e0, e1} of the column-major residual list: G lanes per entry, each lane one
//     16-byte piece of A[row] and of B[col] per K/(4G) step, U entries in flight per lane, xor
//     shuffle reduction (replaces sddmm_gpu_sparse_block_2_2threadOneData_shuffle,
//     sddmmKernel.cu:1994-2104). Entries are ordered by (col % 8, col): consecutive entries
//     share their B column, and slot s is bucket s % 8, so under the round-robin block->XCD
//     dispatch each XCD's L2 serves 1/8 of B plus the (small) A gather.
// The reference launches a panels x ceil(maxBlocks/4) dense grid plus a second kernel on another
// stream; here both parts are one balanced grid with no idle blocks.
// bsmr_sddmm_panels (row-panel shards) uses the panel-major residual items instead, with the
// panel's A rows staged in LDS.
#include <algorithm>
#include <type_traits>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "plan.hpp"
#include "rb_kernel.hpp"
#include "sddmm_device.hpp"

namespace bsmr {
namespace {

struct SddmmArgs {
    const float* A;
    const float* B;
    float* P;
    // dense tiles [d0, d0 + nd) (one tile per wave)
    u32 d0, nd;
    const u32* tileRows;
    const u32* rows;
    u32 R, N, K;
    const u32* denseCols;
    const u32* blockValues;
    // column-major residual slots (full launch)
    const uint2* slots;
    u32 nslots;
    const u32* cmRow;
    const u32* cmCol;
    const u32* cmOut;
    // panel-major residual items (panel ranges)
    const uint4* ritems;
    u32 r0, nr;
    const u32* sparseValues;
    const u32* sparseRel;
    const u32* sparseCol;
    u32 diag;  // profiling ablations (BSMR_DIAG); always 0 in normal use
    unsigned long long* trace;  // BSMR_DIAG & 32: per-wave {start, mid, end, hw id}; else null
    // batched launch (grid.y = batch b): A += b * bA, B += b * bB, P += b * bP (elements)
    unsigned long long bA, bB, bP;
};

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) {
    return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

// ---- one dense tile, K = KT (KT = 0: runtime K, multiple of 16). The tile's 16 A-row indices
// (tileRows), its 16 columns and its 256 output indices depend only on the tile id, so the wave
// has two dependent memory round trips: metadata, then A/B.
template <int KT>
__device__ __forceinline__ void dense_tile(const SddmmArgs& a, const u32 tile) {
    const u32 K = KT > 0 ? KT : a.K;
    const u32 l = __lane_id(), rr = l & 15, g = l >> 4;
    const u32 row = a.tileRows[tile * 16 + rr];
    const u32 c = a.denseCols[tile * 16 + rr];
    const u32* bvals = a.blockValues + static_cast<size_t>(tile) * 256 + 64 * g + rr;
    u32 idx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) idx[r] = bvals[16 * r];
    const bool rvalid = row != NULLV;
    const bool cvalid = c < a.N;
    const float* arow = a.A + static_cast<size_t>(rvalid ? row : 0) * K + 4 * g;
    const float* bcol = a.B + static_cast<size_t>(cvalid ? c : 0) * K + 4 * g;
    f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};  // two chains halve the MFMA dependency
    if constexpr (KT > 0) {
        // chunks of at most 4 k-steps (64 k): 8 float4 = 32 VGPRs of operands in flight, so the
        // kernel fits 64 VGPRs (8 waves per SIMD)
        constexpr int NK = KT / 16;
        constexpr int CH = NK < 4 ? NK : 4;
#pragma unroll
        for (int k0 = 0; k0 < NK; k0 += CH) {
            f32x4 av[CH], bv[CH];
#pragma unroll
            for (int kk = 0; kk < CH; ++kk) {
                av[kk] = rvalid ? ld4(arow + 16 * (k0 + kk)) : f32x4{0, 0, 0, 0};
                bv[kk] = cvalid ? ld4(bcol + 16 * (k0 + kk)) : f32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int kk = 0; kk < CH; ++kk) {
                f32x4& acc = (kk & 1) ? acc1 : acc0;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk].x, bv[kk].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk].y, bv[kk].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk].z, bv[kk].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk].w, bv[kk].w, acc, 0, 0, 0);
            }
        }
    } else {
        for (u32 k = 0; k < K; k += 16) {
            const f32x4 av = rvalid ? ld4(arow + k) : f32x4{0, 0, 0, 0};
            const f32x4 bv = cvalid ? ld4(bcol + k) : f32x4{0, 0, 0, 0};
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc0, 0, 0, 0);
        }
    }
    const f32x4 acc = acc0 + acc1;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (idx[r] != NULLV && (!(a.diag & 1) || acc[r] == -1234.5f)) a.P[idx[r]] = acc[r];
}

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over the 16 lanes of a row, every lane gets the total
__device__ __forceinline__ float row_sum16(float v) {
    v += dppf<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dppf<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dppf<0x141>(v);  // row_half_mirror
    v += dppf<0x140>(v);  // row_mirror
    return v;
}

template <int W>
struct vec;
template <>
struct vec<4> {
    typedef float __attribute__((ext_vector_type(4))) t;
};
template <>
struct vec<2> {
    typedef float __attribute__((ext_vector_type(2))) t;
};
template <>
struct vec<1> {
    typedef float t;
};
template <int W>
__device__ __forceinline__ float vdot(typename vec<W>::t a, typename vec<W>::t b) {
    if constexpr (W == 4)
        return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    else if constexpr (W == 2)
        return a.x * b.x + a.y * b.y;
    else
        return a * b;
}

// ---- column-major residual slot (K = KT known). One 16-lane row per entry: lane s holds the
// W-float pieces s, s+16, ... of A[row] and B[col]. Each row takes a contiguous share of the
// slot's entries (sorted by column); per batch of 16 entries the row loads the metadata once
// (one entry per lane) and broadcasts entry i with row_newbcast:i. U entries are in flight per
// lane; the B pieces are re-loaded only when the column changes (a column run costs one B read);
// the 16-lane dot-product reduction is four DPP adds.
template <int KT>
__device__ __forceinline__ void residual_cm(const SddmmArgs& a, const uint2 sl) {
    constexpr int W = KT >= 64 ? 4 : KT / 16;
    constexpr int NF = KT / (16 * W);
    constexpr int U = NF >= 4 ? 1 : 4 / NF;  // <= 64 VGPRs: 8 waves per SIMD
    typedef typename vec<W>::t vt;
    const u32 l = __lane_id(), sub = l & 15, grp = l >> 4;
    const u32 n = sl.y - sl.x;
    const u32 share = (n + 3) / 4;
    const u32 gs = sl.x + min(grp * share, n), ge = sl.x + min(grp * share + share, n);
    u32 curc = NULLV;
    vt bcur[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) bcur[f] = vt{};
    for (u32 base = gs; base < ge; base += 16) {
        const u32 e = base + sub;
        const bool okm = e < ge;
        const u32 mrow = okm ? a.cmRow[e] : 0u;
        const u32 mcol = okm ? a.cmCol[e] : NULLV;
        const u32 mout = okm ? a.cmOut[e] : 0u;
        const u32 nb = min(16u, ge - base);
#pragma unroll
        for (int i0 = 0; i0 < 16; i0 += U) {
            if (static_cast<u32>(i0) >= nb) break;
            vt av[U][NF], bv[U][NF];
            u32 cc[U], oo[U];
            bool ok[U], chg[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                constexpr int dummy = 0;
                (void)dummy;
                u32 r;
                switch (i0 + u) {  // compile-time lane index after unrolling
#define BSMR_B(I)                    \
    case I:                          \
        r = row_bcast<I>(mrow);      \
        cc[u] = row_bcast<I>(mcol);  \
        oo[u] = row_bcast<I>(mout);  \
        break;
                    BSMR_B(0) BSMR_B(1) BSMR_B(2) BSMR_B(3) BSMR_B(4) BSMR_B(5) BSMR_B(6) BSMR_B(7)
                    BSMR_B(8) BSMR_B(9) BSMR_B(10) BSMR_B(11) BSMR_B(12) BSMR_B(13) BSMR_B(14)
                    BSMR_B(15)
#undef BSMR_B
                    default:
                        r = 0;
                        cc[u] = NULLV;
                        oo[u] = 0;
                }
                ok[u] = static_cast<u32>(i0 + u) < nb;
                const u32 prev = u ? cc[u - 1] : curc;
                chg[u] = ok[u] && cc[u] != prev;
                // a.diag (profiling ablations only; 0 in every real launch): 2 = A row 0, 4 = B col 0
                const u32 ar = (a.diag & 2) ? 0u : (ok[u] ? r : 0u);
                const float* ap = a.A + static_cast<size_t>(ar) * KT + W * sub;
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    av[u][f] = *reinterpret_cast<const vt*>(ap + 16 * W * f);
                if (chg[u]) {
                    const u32 bc = (a.diag & 4) ? 0u : cc[u];
                    const float* bp = a.B + static_cast<size_t>(bc) * KT + W * sub;
#pragma unroll
                    for (int f = 0; f < NF; ++f)
                        bv[u][f] = *reinterpret_cast<const vt*>(bp + 16 * W * f);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!chg[u]) {
#pragma unroll
                    for (int f = 0; f < NF; ++f) bv[u][f] = u ? bv[u - 1][f] : bcur[f];
                }
                float acc = 0.f;
#pragma unroll
                for (int f = 0; f < NF; ++f) acc += vdot<W>(av[u][f], bv[u][f]);
                acc = row_sum16(acc);
                // diag 1: store only an impossible value (keeps the math, drops the P scatter)
                if (sub == 0 && ok[u] && (!(a.diag & 1) || acc == -1234.5f)) a.P[oo[u]] = acc;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (ok[u]) {
                    curc = cc[u];
#pragma unroll
                    for (int f = 0; f < NF; ++f) bcur[f] = bv[u][f];
                }
        }
    }
}

// ---- column-major residual slot, runtime K (multiple of 16): G = 4 lanes per entry
__device__ __forceinline__ void residual_cm_generic(const SddmmArgs& a, const uint2 sl) {
    constexpr u32 G = 4, NG = 16;
    const u32 l = __lane_id(), sub = l % G, grp = l / G;
    const u32 n = sl.y - sl.x;
    const u32 share = (n + NG - 1) / NG;
    const u32 gs = sl.x + min(grp * share, n), ge = sl.x + min(grp * share + share, n);
    for (u32 e = gs; e < ge; ++e) {
        const float* ap = a.A + static_cast<size_t>(a.cmRow[e]) * a.K;
        const float* bp = a.B + static_cast<size_t>(a.cmCol[e]) * a.K;
        float acc = 0.f;
        for (u32 k = 4 * sub; k < a.K; k += 4 * G) acc += dot4(ld4(ap + k), ld4(bp + k));
        acc = group_sum<G>(acc);
        if (sub == 0) a.P[a.cmOut[e]] = acc;
    }
}

// ---- panel-major residual item (panel ranges): A rows of the panel staged in LDS
template <int G>
__device__ __forceinline__ void residual_panel(const SddmmArgs& a, const uint4 it, float* As) {
    const u32 l = __lane_id();
    const u32 K = a.K, KP = K + 4;
    for (u32 x = 4 * l; x < 16 * K; x += 256) {
        const u32 r = x / K, k = x - r * K;
        const u32 q = it.x * 16 + r;
        const f32x4 v = q < a.R ? ld4(a.A + static_cast<size_t>(a.rows[q]) * K + k) : f32x4{0, 0, 0, 0};
        *reinterpret_cast<f32x4*>(As + r * KP + k) = v;
    }
    __syncthreads();
    constexpr u32 EPI = 64 / G;
    const u32 sub = l % G, grp = l / G;
    for (u32 base = it.y; base < it.z; base += EPI) {
        const u32 e = base + grp;
        const bool ok = e < it.z;
        const u32 ee = ok ? e : it.y;
        const float* brow = a.B + static_cast<size_t>(a.sparseCol[ee]) * K;
        const float* arow = As + a.sparseRel[ee] * KP;
        float acc = 0.f;
        for (u32 k = 4 * sub; k < K; k += 4 * G)
            acc += dot4(*reinterpret_cast<const f32x4*>(arow + k), ld4(brow + k));
        acc = group_sum<G>(acc);
        if (sub == 0 && ok) a.P[a.sparseValues[ee]] = acc;
    }
    __syncthreads();
}

// full launch: 256-thread workgroups of four independent waves, one work item per wave (no LDS,
// no barriers); <= 64 VGPRs so 8 waves per SIMD (32 per CU) are resident. Items [0, nd) are dense
// tiles, residual slots start at item ndpad = roundup(nd, 32), so slot s sits in block
// (ndpad + s) / 4 whose XCD (block % 8) is the slot's column bucket (slot layout in plan.hip).
template <int KT, int G>
__global__ __launch_bounds__(256, (KT >= 256 ? 4 : 8)) void k_sddmm_f32(SddmmArgs a) {
    const unsigned long long t0 = rtime(a.trace);
    if (blockIdx.y) {
        a.A += blockIdx.y * a.bA;
        a.B += blockIdx.y * a.bB;
        a.P += blockIdx.y * a.bP;
    }
    const u32 b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b < a.nd) {
        dense_tile<KT>(a, a.d0 + b);
        trace_wave(a.trace, b, t0, t0);
        return;
    }
    const u32 ndpad = (a.nd + 31) & ~31u;
    if (b < ndpad) return;
    const u32 s = b - ndpad;
    if (s < a.nslots) {
        const uint2 sl = a.slots[s];
        if (sl.x < sl.y) {
            if constexpr (KT > 0)
                residual_cm<KT>(a, sl);
            else
                residual_cm_generic(a, sl);
        }
    }
    trace_wave(a.trace, b, t0, t0);
}

// panel-range launch: dense items of the range, then its panel-major residual items
template <int KT, int G>
__global__ __launch_bounds__(64) void k_sddmm_panels_f32(SddmmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float As[];
    const u32 b = blockIdx.x;
    if (b < a.nd) {
        dense_tile<KT>(a, a.d0 + b);
    } else if (b - a.nd < a.nr) {
        residual_panel<G>(a, a.ritems[a.r0 + b - a.nd], As);
    }
}

static_assert(TILES_PER_ITEM == 1, "dense work items are single tiles (tile id = item id)");

using KernelFn = void (*)(SddmmArgs);

template <int G, bool PANELS>
KernelFn pick_k(u32 K) {
#define BSMR_K(KT) (PANELS ? k_sddmm_panels_f32<KT, G> : k_sddmm_f32<KT, G>)
    switch (K) {
        case 32: return BSMR_K(32);
        case 64: return BSMR_K(64);
        case 128: return BSMR_K(128);
        case 256: return BSMR_K(256);
        case 512: return BSMR_K(512);
        default: return BSMR_K(0);
    }
#undef BSMR_K
}

template <bool PANELS>
KernelFn pick_kernel(u32 K) {
    if (K % 64 == 0) return pick_k<16, PANELS>(K);
    if (K % 32 == 0) return pick_k<8, PANELS>(K);
    return pick_k<4, PANELS>(K);
}

int validate(const void* dA, const void* dB, u32 K, int dtype, const float* dP) {
    if (!dA || !dB || !dP) {
        set_error("bsmr_sddmm: null device pointer");
        return BSMR_ERR_INVALID;
    }
    return report(validate_kd("bsmr_sddmm", K, dtype));
}

SddmmArgs make_args(const Plan& p, const void* dA, const void* dB, u32 K, float* dP) {
    SddmmArgs a{};
    a.A = static_cast<const float*>(dA);
    a.B = static_cast<const float*>(dB);
    a.P = dP;
    a.tileRows = p.tileRows.data();
    a.rows = p.rows.data();
    a.R = p.R;
    a.N = p.N;
    a.K = K;
    a.denseCols = p.denseCols.data();
    a.blockValues = p.blockValues.data();
    a.slots = p.cmSlots.data();
    a.cmRow = p.cmRow.data();
    a.cmCol = p.cmCol.data();
    a.cmOut = p.cmOut.data();
    a.ritems = p.resItems.data();
    a.sparseValues = p.sparseValues.data();
    a.sparseRel = p.sparseRel.data();
    a.sparseCol = p.sparseColIdx.data();
    a.diag = p.k.diag;
    return a;
}

// the row-block layout of panels [pa, pb) for slot's row size. A cached layout is returned as it
// is (no HIP call); else it is built now: after lazy_build_guard when a launch asks (at), kept on
// the prepared list when bsmr_plan_prepare_panels does (keep)
int get_rb_layout(const Plan& p, int slot, int dtype, u32 pa, u32 pb,
                  std::shared_ptr<const Plan::RowBlockLayout>* out, const LaunchSite* at = nullptr,
                  bool keep = false) {
    std::lock_guard<std::mutex> g(p.layout_mu);
    const u32 rowBytes = 128u << slot;
    const bool half = dtype != BSMR_F32;
    if (!keep) {
        *out = p.rowblock_ready(rowBytes, half, pa, pb);
        if (*out) return BSMR_OK;
        if (at) BSMR_CHECK(lazy_build_guard(*at));
    }
    int err = BSMR_OK;
    *out = p.rowblock_layout(rowBytes, half, pa, pb, &err, keep);
    return err;
}

// the identity row list of bsmr_sddmm_panels_local (built on first use, as above)
int get_iota(const Plan& p, const LaunchSite* at = nullptr) {
    std::lock_guard<std::mutex> g(p.layout_mu);
    if (p.iotaR.size() >= p.R) return BSMR_OK;
    if (at) BSMR_CHECK(lazy_build_guard(*at));
    std::vector<u32> id(p.R);
    for (u32 q = 0; q < p.R; ++q) id[q] = q;
    BSMR_CHECK(p.iotaR.upload(id.data(), p.R, p.stream));
    BSMR_HIP(hipStreamSynchronize(p.stream));
    return BSMR_OK;
}

// mode: 1 = dense tiles only, 2 = residual only, 3 = both (profiling splits). local: dA holds
// the rows of reordered positions [16 L.pa, L.rowEnd) in that order (row-panel shard with its
// own A rows): the launch stages them through the identity row list, from dA shifted back by
// 16 L.pa rows (addresses only; no row before 16 L.pa is read)
int launch_rb(const Plan& p, const Plan::RowBlockLayout& L, const void* dA, const void* dB,
              float* dP, int dtype, u32 mode, hipStream_t s, u32 nb = 1, bool local = false) {
    if (L.nItems == 0) return BSMR_OK;
    const RbForm f = rb_form(rb_layout_facts(L), p.k, mode);
    RbArgs a{};
    a.A = static_cast<const char*>(dA);
    if (local)
        a.A = reinterpret_cast<const char*>(reinterpret_cast<uintptr_t>(dA) -
                                            static_cast<uintptr_t>(16ull * L.pa * L.rowBytes));
    a.B = static_cast<const char*>(dB);
    // column blocks: B's rows are the staged image, A's the gathered rows (the kernel computes
    // the same dot products with the operands' roles swapped)
    if (L.cols) std::swap(a.A, a.B);
    a.P = dP;
    a.rows = local ? p.iotaR.data() : (L.orig || L.cols) ? L.rowIds.data() : p.rows.data();
    a.row0 = local ? 16 * L.pa : 0;
    a.R = L.rowEnd;
    a.qbase = (L.orig || L.cols) ? 0 : 16 * L.pa;
    a.N = L.cols ? p.M : p.N;
    a.RB = L.RB;
    a.items = L.items.data();
    a.itemEnd = L.itemEnd.data();
    a.pieces = L.pieces.data();
    a.meta = L.meta.data();
    a.out = L.out.data();
    a.outLds = (mode & 2) ? L.outLds : 0u;  // (dense-only profiling launches write no slots)
    a.outPacked = L.outPacked ? 1u : 0u;
    a.stageNt = f.stageNt;
    a.lateB = f.lateB;
    a.stageBlocks = f.stageBlocks ? f.stageBlocks : (L.RB * L.rowBytes + 1023) / 1024;
    a.sortedPos = L.sortedPos.data();
    a.itemEnt = L.itemEnt.data();
    a.runs = L.outRuns ? L.runs.data() : nullptr;
    a.itemRuns = L.outRuns ? L.itemRuns.data() : nullptr;
    a.pairs = f.pairs;
    a.tilePanel = p.denseItems.data();
    a.tileIds = L.tileIds.data();
    a.denseCols = p.denseCols.data();
    a.blockValues = p.blockValues.data();
    a.mode = mode;
    a.diag = p.k.diag;
    if (p.k.diag & 32) {
        BSMR_CHECK(p.prepare_trace(static_cast<size_t>(L.nItems) * (L.NT / 64), s));
        a.trace = p.trace.data();
    }
    a.bA = static_cast<unsigned long long>(L.cols ? p.N : p.M) * L.rowBytes;
    a.bB = static_cast<unsigned long long>(L.cols ? p.M : p.N) * L.rowBytes;
    a.bP = p.nnz;
    void (*fn)(RbArgs) = nullptr;
#define BSMR_RB(DT, RBY) pick_rb<DT, RBY>(f.NT, f.pairs, f.dyn, f.lite)
#define BSMR_RB2(DT)                                                                   \
    (L.rowBytes == 128    ? BSMR_RB(DT, 128)                                              \
     : L.rowBytes == 256  ? BSMR_RB(DT, 256)                                              \
     : L.rowBytes == 512  ? BSMR_RB(DT, 512)                                              \
     : L.rowBytes == 1024 ? BSMR_RB(DT, 1024)                                             \
                          : BSMR_RB(DT, 2048))
    switch (dtype) {
        case BSMR_F32: fn = BSMR_RB2(0); break;
        case BSMR_F16: fn = BSMR_RB2(1); break;
        default: fn = BSMR_RB2(2); break;
    }
#undef BSMR_RB2
#undef BSMR_RB
    hipLaunchKernelGGL(fn, dim3(f.grid, nb), dim3(f.NT), f.ldsBytes, s, a);
    BSMR_HIP(hipGetLastError());
    return BSMR_OK;
}

int launch_full(const Plan& p, SddmmArgs a, hipStream_t s, u32 nb = 1) {
    const u32 items = a.nslots ? ((a.nd + 31) & ~31u) + a.nslots : a.nd;
    if (items == 0) return BSMR_OK;
    a.bA = static_cast<unsigned long long>(p.M) * a.K;
    a.bB = static_cast<unsigned long long>(p.N) * a.K;
    a.bP = p.nnz;
    if (p.k.diag & 32) {
        BSMR_CHECK(p.prepare_trace((items + 3) / 4 * 4, s));
        a.trace = p.trace.data();
    }
    hipLaunchKernelGGL(pick_kernel<false>(a.K), dim3((items + 3) / 4, nb), dim3(256), 0, s, a);
    BSMR_HIP(hipGetLastError());
    return BSMR_OK;
}

int launch_panels(SddmmArgs a, hipStream_t s) {
    const u32 grid = a.nd + a.nr;
    if (grid == 0) return BSMR_OK;
    const size_t lds = a.nr ? static_cast<size_t>(16) * (a.K + 4) * sizeof(float) : 0;
    hipLaunchKernelGGL(pick_kernel<true>(a.K), dim3(grid), dim3(64), lds, s, a);
    BSMR_HIP(hipGetLastError());
    return BSMR_OK;
}

}  // namespace

static const char* dtype_name(int dtype) {
    return dtype == BSMR_F32 ? "fp32" : dtype == BSMR_F16 ? "fp16" : "bf16";
}

// A launch found its layout not built. Building allocates, copies and synchronises, none of which
// a capturing stream survives, so the launch is refused there (the one HIP call made is the query).
int lazy_build_guard(const LaunchSite& at) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(at.s, &cs);
    if (e != hipSuccess) {
        set_error(std::string(at.who) + ": hipStreamIsCapturing: " + hipGetErrorString(e));
        return BSMR_ERR_HIP;
    }
    if (cs == hipStreamCaptureStatusNone) return BSMR_OK;
    set_error(std::string(at.who) + ": stream is capturing and the layout of (K = " +
              std::to_string(at.K) + ", " + dtype_name(at.dtype) + ") is not built; call " + at.prep +
              " first");
    return BSMR_ERR_NOT_PREPARED;
}

// the whole plan's row-block layout for (K, dtype), built on first use; *out = null when that
// (K, dtype) runs the column-major launch
int whole_rb_layout(const Plan& p, u32 K, int dtype, const Plan::RowBlockLayout** out,
                    bool reordered) {
    *out = nullptr;
    const LaunchChoice c = choose_launch(p, K, dtype);
    if (c.slot < 0 || c.kind == Launch::Ptile) return BSMR_OK;
    std::shared_ptr<const Plan::RowBlockLayout> L;  // the whole plan's: a plan member
    BSMR_CHECK(get_rb_layout(p, c.slot, dtype, 0, p.P, &L));
    *out = L.get();
    if (reordered && (L->orig || L->cols)) *out = &p.rb_reordered(c.slot, dtype);
    return BSMR_OK;
}

}  // namespace bsmr

using namespace bsmr;

// one launch per at most 65535 batches (grid.y); batch b reads A + b*M*K, B + b*N*K and writes
// P + b*nnz (sddmm_gpu_batch, sddmmKernel.cu:2764-2850)
static int sddmm_batch(const char* who, const bsmr_plan* plan, uint32_t num_batch, const void* dA,
                       const void* dB, uint32_t K, int dtype, float* dP, void* stream) {
    if (!plan) {
        set_error("bsmr_sddmm: null plan");
        return BSMR_ERR_INVALID;
    }
    if (num_batch == 0) {
        set_error("bsmr_sddmm_batch: num_batch must be >= 1");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    BSMR_CHECK(validate(dA, dB, K, dtype, dP));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t es = dtype == BSMR_F32 ? 4 : 2;
    const LaunchSite at{s, who, "bsmr_plan_prepare", K, dtype};
    const LaunchChoice c = choose_launch(p, K, dtype);
    for (u32 b0 = 0; b0 < num_batch; b0 += 65535u) {
        const u32 nb = std::min<u32>(num_batch - b0, 65535u);
        const char* A = static_cast<const char*>(dA) + es * b0 * static_cast<size_t>(p.M) * K;
        const char* B = static_cast<const char*>(dB) + es * b0 * static_cast<size_t>(p.N) * K;
        float* P = dP + static_cast<size_t>(b0) * p.nnz;
        switch (c.kind) {
            case Launch::Ptile: BSMR_CHECK(launch_ptile(p, A, B, K, dtype, P, 3, s, nb, &at)); break;
            case Launch::Dense: BSMR_CHECK(launch_dense(p, A, B, K, dtype, P, s, nb, &at)); break;
            case Launch::RowBlock: {
                std::shared_ptr<const Plan::RowBlockLayout> L;
                BSMR_CHECK(get_rb_layout(p, c.slot, dtype, 0, p.P, &L, &at));
                BSMR_CHECK(launch_rb(p, *L, A, B, P, dtype, 3, s, nb));
                break;
            }
            case Launch::Half: BSMR_CHECK(launch_half(p, A, B, K, dtype, P, 3, s, nb)); break;
            case Launch::ColMajor: {
                SddmmArgs a = make_args(p, A, B, K, P);
                a.nd = p.nDenseItems;
                a.nslots = p.nSlots;
                BSMR_CHECK(launch_full(p, a, s, nb));
            }
        }
    }
    return BSMR_OK;
}

extern "C" int bsmr_sddmm_batch(const bsmr_plan* plan, uint32_t num_batch, const void* dA,
                                const void* dB, uint32_t K, int dtype, float* dP, void* stream) {
    return sddmm_batch("bsmr_sddmm_batch", plan, num_batch, dA, dB, K, dtype, dP, stream);
}

extern "C" int bsmr_sddmm(const bsmr_plan* plan, const void* dA, const void* dB, uint32_t K,
                          int dtype, float* dP, void* stream) {
    return sddmm_batch("bsmr_sddmm", plan, 1, dA, dB, K, dtype, dP, stream);
}

// the plan's choice for (K, dtype) and the panel-range rules, for the four panel entry points
static int panel_choice(const char* who, const Plan& p, u32 K, int dtype, u32 p0, u32 p1, bool local,
                        LaunchChoice* c) {
    *c = choose_launch(p, K, dtype);
    return report(check_panel_range(who, p0, p1, p.P, c->slot, dtype, local));
}

extern "C" int bsmr_sddmm_panels(const bsmr_plan* plan, const void* dA, const void* dB,
                                 uint32_t K, int dtype, float* dP, uint32_t p0, uint32_t p1,
                                 void* stream) {
    if (!plan) {
        set_error("bsmr_sddmm_panels: null plan");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    BSMR_CHECK(validate(dA, dB, K, dtype, dP));
    LaunchChoice c;
    BSMR_CHECK(panel_choice("bsmr_sddmm_panels", p, K, dtype, p0, p1, false, &c));
    if (p0 == p1) return BSMR_OK;
    // the row-block kernel over the range's own layout (same kernel as the whole plan)
    if (c.slot >= 0) {
        const LaunchSite at{static_cast<hipStream_t>(stream), "bsmr_sddmm_panels",
                            "bsmr_plan_prepare_panels", K, dtype};
        std::shared_ptr<const Plan::RowBlockLayout> L;  // held until the launch is enqueued
        BSMR_CHECK(get_rb_layout(p, c.slot, dtype, p0, p1, &L, &at));
        return launch_rb(p, *L, dA, dB, dP, dtype, 3, at.s);
    }
    // items are stored panel-major: ceil(tiles_q / TILES_PER_ITEM) dense and
    // ceil(nres_q / RES_PER_ITEM) residual items per panel q
    u32 d0 = 0, d1 = 0, r0 = 0, r1 = 0;
    for (u32 q = 0; q < p1; ++q) {
        const u32 nt = p.h_blockOffsets[q + 1] - p.h_blockOffsets[q];
        const u32 ne = p.h_sparseValueOffsets[q + 1] - p.h_sparseValueOffsets[q];
        const u32 di = (nt + TILES_PER_ITEM - 1) / TILES_PER_ITEM;
        const u32 ri = (ne + RES_PER_ITEM - 1) / RES_PER_ITEM;
        if (q < p0) {
            d0 += di;
            r0 += ri;
        }
        d1 += di;
        r1 += ri;
    }
    SddmmArgs a = make_args(p, dA, dB, K, dP);
    a.d0 = d0;
    a.nd = d1 - d0;
    a.r0 = r0;
    a.nr = r1 - r0;
    return launch_panels(a, static_cast<hipStream_t>(stream));
}

extern "C" int bsmr_sddmm_panels_local(const bsmr_plan* plan, const void* dA_local,
                                       const void* dB, uint32_t K, int dtype, float* dP,
                                       uint32_t p0, uint32_t p1, void* stream) {
    if (!plan) {
        set_error("bsmr_sddmm_panels_local: null plan");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    BSMR_CHECK(validate(dA_local, dB, K, dtype, dP));
    LaunchChoice c;
    BSMR_CHECK(panel_choice("bsmr_sddmm_panels_local", p, K, dtype, p0, p1, true, &c));
    if (p0 == p1) return BSMR_OK;
    const LaunchSite at{static_cast<hipStream_t>(stream), "bsmr_sddmm_panels_local",
                        "bsmr_plan_prepare_panels", K, dtype};
    BSMR_CHECK(get_iota(p, &at));
    std::shared_ptr<const Plan::RowBlockLayout> L;  // held until the launch is enqueued
    BSMR_CHECK(get_rb_layout(p, c.slot, dtype, p0, p1, &L, &at));
    if (L->orig || L->cols)  // the whole range may have picked original-order row blocks or
                             // column blocks: use the reordered layout, whose rows follow the local A
        L = std::shared_ptr<const Plan::RowBlockLayout>(std::shared_ptr<void>(),
                                                        &p.rb_reordered(c.slot, dtype));
    return launch_rb(p, *L, dA_local, dB, dP, dtype, 3, at.s, 1, true);
}

// ---- explicit layout builds (bsmr.h): what the launches above would build on first use ----

static int prepare_args(const char* who, const bsmr_plan* plan, uint32_t K, int dtype) {
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    return report(validate_kd(who, K, dtype));
}

// the panel-range checks of bsmr_sddmm_panels / _panels_local; *slot = -1 when there is nothing
// to build (an empty range, or fp32 on the panel-major lists)
static int prepare_panels_args(const char* who, const bsmr_plan* plan, uint32_t K, int dtype,
                               uint32_t p0, uint32_t p1, int local, int* slot) {
    *slot = -1;
    BSMR_CHECK(prepare_args(who, plan, K, dtype));
    LaunchChoice c;
    BSMR_CHECK(panel_choice(who, plan->p, K, dtype, p0, p1, local != 0, &c));
    if (p0 != p1) *slot = c.slot;
    return BSMR_OK;
}

extern "C" int bsmr_plan_prepare(const bsmr_plan* plan, uint32_t K, int dtype) {
    BSMR_CHECK(prepare_args("bsmr_plan_prepare", plan, K, dtype));
    const Plan& p = plan->p;
    const LaunchChoice c = choose_launch(p, K, dtype);
    BSMR_CHECK(report(validate_launch_k("bsmr_plan_prepare", c.kind, K)));
    switch (c.kind) {
        case Launch::Ptile: {
            std::lock_guard<std::mutex> g(p.layout_mu);
            if (!p.ptile_ready()) BSMR_CHECK(p.build_ptile_layout(p.k.ptile_tpi));
            return BSMR_OK;
        }
        case Launch::Dense: {
            std::lock_guard<std::mutex> g(p.layout_mu);
            if (!p.dense.built) BSMR_CHECK(p.build_dense_layout());
            return BSMR_OK;
        }
        case Launch::RowBlock: {
            std::shared_ptr<const Plan::RowBlockLayout> L;
            return get_rb_layout(p, c.slot, dtype, 0, p.P, &L);
        }
        default: return BSMR_OK;  // the column-major lists are the plan's own
    }
}

extern "C" int bsmr_plan_prepared(const bsmr_plan* plan, uint32_t K, int dtype) {
    if (prepare_args("bsmr_plan_prepared", plan, K, dtype) != BSMR_OK) return 0;
    const Plan& p = plan->p;
    const LaunchChoice c = choose_launch(p, K, dtype);
    const Launch kind = c.kind;
    if (report(validate_launch_k("bsmr_plan_prepared", kind, K)) != BSMR_OK) return 0;
    if (kind == Launch::Half || kind == Launch::ColMajor) return 1;
    std::lock_guard<std::mutex> g(p.layout_mu);
    if (kind == Launch::Ptile) return p.ptile_ready();
    if (kind == Launch::Dense) return p.dense.built;
    return p.rowblock_ready(c.rowBytes, dtype != BSMR_F32, 0, p.P) != nullptr;
}

extern "C" int bsmr_plan_prepare_panels(const bsmr_plan* plan, uint32_t K, int dtype, uint32_t p0,
                                        uint32_t p1, int local) {
    int slot = -1;
    BSMR_CHECK(prepare_panels_args("bsmr_plan_prepare_panels", plan, K, dtype, p0, p1, local, &slot));
    if (slot < 0) return BSMR_OK;
    const Plan& p = plan->p;
    if (local) BSMR_CHECK(get_iota(p));
    std::shared_ptr<const Plan::RowBlockLayout> L;
    return get_rb_layout(p, slot, dtype, p0, p1, &L, nullptr, true);
}

extern "C" int bsmr_plan_panels_prepared(const bsmr_plan* plan, uint32_t K, int dtype, uint32_t p0,
                                         uint32_t p1, int local) {
    int slot = -1;
    if (prepare_panels_args("bsmr_plan_panels_prepared", plan, K, dtype, p0, p1, local, &slot) != BSMR_OK)
        return 0;
    if (slot < 0) return 1;
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    if (local && p.iotaR.size() < p.R) return 0;
    return p.rowblock_ready(128u << slot, dtype != BSMR_F32, p0, p1) != nullptr;
}

extern "C" int bsmr_sddmm_profile(const bsmr_plan* plan, const void* dA, const void* dB,
                                  uint32_t K, int dtype, float* dP, int iters, void* stream,
                                  float* ms_dense, float* ms_residual, float* ms_total) {
    if (!plan || iters <= 0) {
        set_error("bsmr_sddmm_profile: bad arguments");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    BSMR_CHECK(validate(dA, dB, K, dtype, dP));
    hipStream_t s = static_cast<hipStream_t>(stream);
    {  // the timing synchronises events: never on a capturing stream
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        BSMR_HIP(hipStreamIsCapturing(s, &cs));
        if (cs != hipStreamCaptureStatusNone) {
            set_error("bsmr_sddmm_profile: stream is capturing (the timing synchronises events)");
            return BSMR_ERR_UNSUPPORTED;
        }
    }
    struct Events {  // destroyed on every return path
        hipEvent_t e[4] = {};
        ~Events() {
            for (auto& x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } evs;
    hipEvent_t* ev = evs.e;
    for (int i = 0; i < 4; ++i) BSMR_HIP(hipEventCreate(&ev[i]));
    const LaunchChoice c = choose_launch(p, K, dtype);
    std::shared_ptr<const Plan::RowBlockLayout> L;
    if (c.kind == Launch::RowBlock) BSMR_CHECK(get_rb_layout(p, c.slot, dtype, 0, p.P, &L));
    SddmmArgs full = make_args(p, dA, dB, K, dP);
    full.nd = p.nDenseItems;
    full.nslots = p.nSlots;
    SddmmArgs dense = full;
    dense.nslots = 0;
    SddmmArgs res = full;
    res.nd = 0;
    auto run = [&](u32 mode) -> int {
        switch (c.kind) {
            case Launch::Ptile: return launch_ptile(p, dA, dB, K, dtype, dP, mode, s);
            case Launch::Dense: return launch_dense(p, dA, dB, K, dtype, dP, s);  // no dense/residual split
            case Launch::RowBlock: return launch_rb(p, *L, dA, dB, dP, dtype, mode, s);
            case Launch::Half: return launch_half(p, dA, dB, K, dtype, dP, mode, s);
            default: return launch_full(p, mode == 1 ? dense : mode == 2 ? res : full, s);
        }
    };
    BSMR_HIP(hipEventRecord(ev[0], s));
    for (int i = 0; i < iters; ++i) BSMR_CHECK(run(1));
    BSMR_HIP(hipEventRecord(ev[1], s));
    for (int i = 0; i < iters; ++i) BSMR_CHECK(run(2));
    BSMR_HIP(hipEventRecord(ev[2], s));
    for (int i = 0; i < iters; ++i) BSMR_CHECK(run(3));
    BSMR_HIP(hipEventRecord(ev[3], s));
    BSMR_HIP(hipEventSynchronize(ev[3]));
    float t0 = 0, t1 = 0, t2 = 0;
    BSMR_HIP(hipEventElapsedTime(&t0, ev[0], ev[1]));
    BSMR_HIP(hipEventElapsedTime(&t1, ev[1], ev[2]));
    BSMR_HIP(hipEventElapsedTime(&t2, ev[2], ev[3]));
    if (ms_dense) *ms_dense = p.nDenseItems ? t0 / iters : 0.f;
    if (ms_residual) *ms_residual = p.nres ? t1 / iters : 0.f;
    if (ms_total) *ms_total = t2 / iters;
    return BSMR_OK;
}

// debug: the whole-plan row-block layout of (K, dtype), 4 u32 per item slot in launch order
// {row block, kept tiles, entries, pieces} (padding slots all zero), preceded by the header
// {rows per block, threads per workgroup, items, row bytes}; *len = 4 (items + 1). Not in the
// header (tools/item_trace.py)
extern "C" int bsmr_debug_rb_items(const bsmr_plan* plan, uint32_t K, int dtype, uint32_t* host_out,
                                   uint64_t* len) {
    if (!plan) return BSMR_ERR_INVALID;
    const Plan& p = plan->p;
    const Plan::RowBlockLayout* L = nullptr;
    BSMR_CHECK(whole_rb_layout(p, K, dtype, &L));
    if (!L) {
        if (len) *len = 0;
        return BSMR_OK;
    }
    if (len) *len = 4ull * (L->itemStat.size() + 1);
    if (host_out) {
        host_out[0] = L->RB;
        host_out[1] = L->NT;
        host_out[2] = static_cast<uint32_t>(L->itemStat.size());
        host_out[3] = L->rowBytes;
        for (size_t i = 0; i < L->itemStat.size(); ++i) {
            const uint4 v = L->itemStat[i];
            host_out[4 * (i + 1) + 0] = v.x;
            host_out[4 * (i + 1) + 1] = v.y;
            host_out[4 * (i + 1) + 2] = v.z;
            host_out[4 * (i + 1) + 3] = v.w;
        }
    }
    return BSMR_OK;
}

// debug: the whole plan's row-block layout for (K, dtype) as {items (4 u32 each: row block, tile
// begin, tile end, piece begin), item ends, pieces (2 u32 each)}: *len = 4 n + n + 2 p + 2 with
// host_out[0] = n items, [1] = p pieces (tools/phase_balance.py; not in the header)
extern "C" int bsmr_debug_rb_pieces(const bsmr_plan* plan, uint32_t K, int dtype, uint32_t* host_out,
                                    uint64_t* len) {
    if (!plan) return BSMR_ERR_INVALID;
    const Plan& p = plan->p;
    const Plan::RowBlockLayout* L = nullptr;
    BSMR_CHECK(whole_rb_layout(p, K, dtype, &L));
    const u64 n = L ? L->nItems : 0, np = L ? L->nPieces : 0;
    if (len) *len = 2 + 5 * n + 2 * np;
    if (host_out && L) {
        host_out[0] = static_cast<uint32_t>(n);
        host_out[1] = static_cast<uint32_t>(np);
        BSMR_HIP(hipMemcpy(host_out + 2, L->items.data(), n * sizeof(uint4), hipMemcpyDeviceToHost));
        BSMR_HIP(hipMemcpy(host_out + 2 + 4 * n, L->itemEnd.data(), n * sizeof(u32), hipMemcpyDeviceToHost));
        BSMR_HIP(hipMemcpy(host_out + 2 + 5 * n, L->pieces.data(), np * sizeof(uint2), hipMemcpyDeviceToHost));
    }
    return BSMR_OK;
}

namespace {
// the store export of layout L (bsmr_debug_rb_store; ext: the panel-range form of
// bsmr_debug_rb_store_panels, whose header also holds the launch's form and whose item words
// also hold the row block and whether the item is real)
int store_export(const Plan& p, const Plan::RowBlockLayout& L, bool ext, uint32_t* host_out, uint64_t* len) {
    const u64 cap = host_out ? *len : 0;
    const u64 n = L.nItems;
    const bool staged = L.outLds != 0;
    std::vector<uint2> ient, irun, runs;
    std::vector<u32> spos, iend;
    std::vector<uint4> items;
    if (staged) {
        BSMR_CHECK(L.itemEnt.download(ient, p.stream));
        if (L.outRuns) {
            BSMR_CHECK(L.itemRuns.download(irun, p.stream));
            BSMR_CHECK(L.runs.download(runs, p.stream));
            u64 nr = 0;
            for (u64 i = 0; i < n; ++i) nr += irun[i].y;
            runs.resize(nr);  // (an empty table is uploaded as one word)
        } else {
            BSMR_CHECK(L.sortedPos.download(spos, p.stream));
            spos.resize(L.nEntries);
        }
        ient.resize(n);
    }
    if (ext) {
        BSMR_CHECK(L.items.download(items, p.stream));
        BSMR_CHECK(L.itemEnd.download(iend, p.stream));
        items.resize(n);
        iend.resize(n);
    }
    const u64 nh = ext ? 12 : 8, per = ext ? 6 : 4;
    const u64 head = nh + per * n;
    const u64 full = head + (staged ? 2 * n + (L.outRuns ? 2 * n + 2 * runs.size() : spos.size()) : 0);
    *len = full;
    if (!host_out || cap < head) return BSMR_OK;
    const RbForm f = rb_form(rb_layout_facts(L), p.k, 3);
    const u32 hdr[12] = {L.outLds, L.outCap, L.outRuns, L.outPacked, L.NT, static_cast<u32>(n),
                         PAIR_RUNS_PER_WAVE, XCD_BUCKETS, f.pairs, f.dyn, f.lite, f.grid};
    std::copy(hdr, hdr + nh, host_out);
    for (u64 i = 0; i < n; ++i) {
        u32* w = host_out + nh + per * i;
        w[0] = staged ? ient[i].y : (i < L.itemStat.size() ? L.itemStat[i].z : 0u);
        w[1] = w[2] = w[3] = 0;
        if (staged && L.outRuns) {
            w[1] = irun[i].y;
            for (u32 r = irun[i].x; r < irun[i].x + irun[i].y; ++r) {
                const u32 l = runs[r].y >> 16;
                w[2] = std::max(w[2], l);
                w[3] = r == irun[i].x ? l : std::min(w[3], l);
            }
        }
        if (ext) {
            w[4] = items[i].x;
            w[5] = !(items[i].y == items[i].z && items[i].w == iend[i]);  // (k_sddmm_rb's padding test)
        }
    }
    if (!staged || cap < full) return BSMR_OK;
    u32* w = host_out + head;
    for (u64 i = 0; i < n; ++i) { *w++ = ient[i].x; *w++ = ient[i].y; }
    if (L.outRuns) {
        for (u64 i = 0; i < n; ++i) { *w++ = irun[i].x; *w++ = irun[i].y; }
        for (const uint2& r : runs) { *w++ = r.x; *w++ = r.y; }
    } else {
        std::copy(spos.begin(), spos.end(), w);
    }
    return BSMR_OK;
}
}  // namespace

// debug: how the whole-plan row-block layout of (K, dtype) writes P. host_out = the header {outLds,
// outCap, outRuns, outPacked, NT, n item slots, PAIR_RUNS_PER_WAVE, XCD_BUCKETS}, then 4 u32 per
// item slot in launch order {entries (itemEnt.y; unstaged: the item's entry count), runs
// (itemRuns.y; 0 without a run table), longest run, shortest run (0 without runs)}, then the raw
// tables of a staged layout: itemEnt (2 u32 per item: first entry, entries) and, with a run table,
// itemRuns (2 u32 per item) and the r run words (2 u32 each), else sortedPos (one u32 per entry).
// *len on entry = the u32 the buffer holds, on return = those of the whole export; the raw tables
// are written only into a buffer that holds all of it (the header and the item words into one of
// 8 + 4 n). *len = 0 without a row-block layout. Not in the header (tests/gpu_util.py rb_store)
extern "C" int bsmr_debug_rb_store(const bsmr_plan* plan, uint32_t K, int dtype, uint32_t* host_out,
                                   uint64_t* len) {
    if (!plan || !len) return BSMR_ERR_INVALID;
    const Plan& p = plan->p;
    const Plan::RowBlockLayout* L = nullptr;
    BSMR_CHECK(whole_rb_layout(p, K, dtype, &L));
    if (!L) {
        *len = 0;
        return BSMR_OK;
    }
    return store_export(p, *L, false, host_out, len);
}

// debug: the same for the layout bsmr_sddmm_panels runs over panels [p0, p1) (the range's own
// layout, built on first use as the launch builds it), with the launch's form: the header has 12
// words, the eight above and {pairs, dynamic batches, lite, grid} of rb_form on that layout, and
// an item slot has 6, the four above and {row block, 1 if the item is real (0: padding)}. *len = 0
// when (K, dtype) has no row-block slot or the range is empty. Not in the header
extern "C" int bsmr_debug_rb_store_panels(const bsmr_plan* plan, uint32_t K, int dtype, uint32_t p0,
                                          uint32_t p1, uint32_t* host_out, uint64_t* len) {
    if (!plan || !len) return BSMR_ERR_INVALID;
    const Plan& p = plan->p;
    LaunchChoice c;
    BSMR_CHECK(panel_choice("bsmr_debug_rb_store_panels", p, K, dtype, p0, p1, false, &c));
    if (c.slot < 0 || p0 == p1) {
        *len = 0;
        return BSMR_OK;
    }
    std::shared_ptr<const Plan::RowBlockLayout> L;
    BSMR_CHECK(get_rb_layout(p, c.slot, dtype, p0, p1, &L));
    return store_export(p, *L, true, host_out, len);
}

// debug: the store pass's constants {PAIR_RUNS_PER_WAVE, XCD_BUCKETS, RB_RUN_MAX}, for a host
// model of a layout. Needs no device. Not in the header (tests/test_store_ref_cpu.py)
extern "C" int bsmr_debug_rb_store_constants(uint32_t* out) {
    if (!out) return BSMR_ERR_INVALID;
    out[0] = PAIR_RUNS_PER_WAVE;
    out[1] = XCD_BUCKETS;
    out[2] = RB_RUN_MAX;
    return BSMR_OK;
}

// debug timeline of the last traced launch (BSMR_DIAG & 32): 4 u64 per wave (not in the header)
extern "C" int bsmr_debug_trace(const bsmr_plan* plan, uint64_t* host_out, uint64_t* len) {
    if (!plan) return BSMR_ERR_INVALID;
    const Plan& p = plan->p;
    if (len) *len = p.traceN * 4ull;
    if (host_out && p.traceN) {
        BSMR_HIP(hipDeviceSynchronize());
        BSMR_HIP(hipMemcpy(host_out, p.trace.data(), p.traceN * 4ull * sizeof(uint64_t),
                           hipMemcpyDeviceToHost));
    }
    return BSMR_OK;
}
