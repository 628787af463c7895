// spmm.hip — plan-based SpMM for gfx950: Y = S(V) B (bsmr_spmm, rows of S) and Y = S(V)^T A
// (bsmr_spmm_t, columns of S), the gradients dA / dB of bsmr_sddmm when V = dP.
//
// One wave per segment of a destination's gather list (spmm_schedule.cpp). A dense row of
// rowBytes = K * sizeof(T) is covered by rowBytes / 16 lanes with 16-byte loads; for rows under
// 1 KiB the other lane groups of the wave take further entries of the segment in the same
// instruction, for 2 KiB rows a lane takes two chunks. fp32 accumulation with one FMA per term,
// lane groups reduced in a fixed butterfly, fp32 stores. No atomics: a destination whose list is
// longer than `chunk` writes one partial row per segment to plan-owned scratch, and k_spmm_reduce
// adds the partials in chunk order, so results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "plan.hpp"
#include "row_elems.hpp"
#include "spmm_schedule.hpp"

namespace bsmr {
namespace {

// Both are macros so that an A/B build can override them (-D...). Measured, dA / dB:
// 16 waves, 4 chunks: C2 29.6 / 32.0 us, C3 129.9 / 128.6 us; 8 chunks (106 VGPRs, 4 waves per
// SIMD): 30.4 / 32.0 and 156.8 / 166.8; 4 waves per workgroup: 28.3 / 29.9 and 159.3 / 138.4
#ifndef SPMM_WAVES_PER_WG
#define SPMM_WAVES_PER_WG 16
#endif
constexpr u32 SPMM_WAVES = SPMM_WAVES_PER_WG;  // waves (segments) per workgroup: one 16-row panel of the order
#ifndef SPMM_UNROLL
#define SPMM_UNROLL 4  // 16-byte row chunks a lane keeps in flight
#endif

struct SpmmArgs {
    const SpmmSeg* segs;
    const u32* src;
    const u32* vpos;
    const float* V;
    const char* X;     // gathered operand, rows of rowBytes
    float* Y;          // destinations x K
    float* partial;    // partial slots x K
    u32 nSegs, K, rowBytes;
    u32 lanes;         // generic form: lanes per row (a power of two <= 64)
};

// LANES: lanes per row, compile-time (8, 16, 32, 64) or 0 = a.lanes (generic form, rows of any
// multiple of 16 bytes: lanes past the row idle, rows over 1 KiB go in 1-KiB column tiles).
// CH: 16-byte chunks per lane (2 for 2 KiB rows: the second at +1 KiB).
template <int DT, int LANES, int CH>
__global__ __launch_bounds__(SPMM_WAVES * 64) void k_spmm(const SpmmArgs a) {
    using E = Elem<DT>;
    constexpr int EPL = E::EPL;
    const u32 lane = threadIdx.x & 63u;
    // the wave's segment, wave-uniform (scalar loads of its descriptor, scalar loop counters)
    const u32 segId = blockIdx.x * SPMM_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (segId >= a.nSegs) return;
    const SpmmSeg sg = a.segs[segId];
    const u32 L = LANES ? static_cast<u32>(LANES) : a.lanes;
    const u32 G = 64u / L;              // entries per instruction
    const u32 g = lane / L, l = lane % L;
    const u32 rowChunks = a.rowBytes / 16u;
    float* out = sg.part == SPMM_DIRECT ? a.Y + static_cast<size_t>(sg.dst) * a.K
                                        : a.partial + static_cast<size_t>(sg.part) * a.K;
    const u32* src = a.src + sg.first;
    const u32* vpos = a.vpos + sg.first;
    // column tiles of 64 chunks: one for every fixed size (CH chunks per lane), rows over 1 KiB
    // of the generic form take several
    const u32 tiles = LANES ? 1u : (rowChunks + 63u) / 64u;
    for (u32 t = 0; t < tiles; ++t) {
        const u32 c0 = t * 64u + l;  // this lane's first chunk of the row
        const bool live = LANES ? true : c0 < rowChunks;
        float acc[CH][EPL];
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int i = 0; i < EPL; ++i) acc[c][i] = 0.f;
        // a batch's indices and values, one entry per lane; the next batch's are loaded under the
        // current one's gathers
        auto batch = [&](u32 b, u32& ms, float& mv) {
            ms = 0;
            mv = 0.f;
            if (b + lane < sg.count) {
                ms = src[b + lane];
                mv = a.V[vpos[b + lane]];
            }
        };
        u32 ms, nms = 0;
        float mv, nmv = 0.f;
        batch(0, ms, mv);
        for (u32 b = 0; b < sg.count; b += 64u) {
            const u32 nb = min(64u, sg.count - b);
            if (b + 64u < sg.count) batch(b + 64u, nms, nmv);
            const u32 full = nb / G;  // steps in which every lane group has an entry
            // every lane takes part in the shuffles (an idle lane may hold another's entry); only
            // the loads and the FMAs are predicated
            auto pick = [&](u32 idx, u32& s, float& v) {
                s = __shfl(ms, static_cast<int>(idx & 63u));
                v = __shfl(mv, static_cast<int>(idx & 63u));
            };
            auto load = [&](u32 s, uint4* q) {
                const char* row = a.X + static_cast<size_t>(s) * a.rowBytes + static_cast<size_t>(c0) * 16u;
#pragma unroll
                for (int c = 0; c < CH; ++c) q[c] = *reinterpret_cast<const uint4*>(row + c * 1024);
            };
            auto fma = [&](float v, const uint4* q) {
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    float x[EPL];
                    E::unpack(q[c], x);
#pragma unroll
                    for (int i = 0; i < EPL; ++i) acc[c][i] = __builtin_fmaf(v, x[i], acc[c][i]);
                }
            };
            // U steps' rows in flight at once (32 VGPRs of loads), then their FMAs in entry order
            constexpr u32 U = SPMM_UNROLL / CH;
            u32 j = 0;
            for (; j + U <= full; j += U) {
                u32 s[U];
                float v[U];
                uint4 q[U][CH];
#pragma unroll
                for (u32 u = 0; u < U; ++u) pick((j + u) * G + g, s[u], v[u]);
                if (live) {
#pragma unroll
                    for (u32 u = 0; u < U; ++u) load(s[u], q[u]);
#pragma unroll
                    for (u32 u = 0; u < U; ++u) fma(v[u], q[u]);
                }
            }
            for (; j * G < nb; ++j) {  // the remaining steps; the last may be partly filled
                const u32 idx = j * G + g;
                u32 s;
                float v;
                uint4 q[CH];
                pick(idx, s, v);
                if (live && idx < nb) {
                    load(s, q);
                    fma(v, q);
                }
            }
            ms = nms;
            mv = nmv;
        }
        // lane groups in a fixed butterfly (group g held entries g, g + G, ... of the segment)
        for (u32 off = 32u; off >= L; off >>= 1)
#pragma unroll
            for (int c = 0; c < CH; ++c)
#pragma unroll
                for (int i = 0; i < EPL; ++i) acc[c][i] += __shfl_xor(acc[c][i], static_cast<int>(off));
        if (g == 0 && live) {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                float* o = out + (static_cast<size_t>(c0) + c * 64u) * EPL;
#pragma unroll
                for (int i = 0; i < EPL; i += 4)
                    *reinterpret_cast<float4*>(o + i) =
                        make_float4(acc[c][i], acc[c][i + 1], acc[c][i + 2], acc[c][i + 3]);
            }
        }
    }
}

// Y[dst] = the destination's partial rows added in chunk order; one thread per four columns
__global__ __launch_bounds__(256) void k_spmm_reduce(const SpmmRed* reds, u32 nReds, const float* partial,
                                                     float* Y, u32 K) {
    const u32 q4 = K / 4u;
    const size_t t = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= static_cast<size_t>(nReds) * q4) return;
    const SpmmRed r = reds[t / q4];
    const u32 q = static_cast<u32>(t % q4);
    const float4* p = reinterpret_cast<const float4*>(partial + static_cast<size_t>(r.part0) * K) + q;
    float4 s = p[0];
    for (u32 i = 1; i < r.nparts; ++i) {
        const float4 x = p[static_cast<size_t>(i) * q4];
        s.x += x.x;
        s.y += x.y;
        s.z += x.z;
        s.w += x.w;
    }
    reinterpret_cast<float4*>(Y + static_cast<size_t>(r.dst) * K)[q] = s;
}

using SpmmFn = void (*)(const SpmmArgs);

template <int DT>
SpmmFn pick_spmm(u32 rowBytes) {
    switch (rowBytes) {
        case 128: return k_spmm<DT, 8, 1>;
        case 256: return k_spmm<DT, 16, 1>;
        case 512: return k_spmm<DT, 32, 1>;
        case 1024: return k_spmm<DT, 64, 1>;
        case 2048: return k_spmm<DT, 64, 2>;
        default: return k_spmm<DT, 0, 1>;
    }
}

const char* side_call(int side) { return side == 1 ? "bsmr_spmm" : "bsmr_spmm_t"; }

// a side's lists and scratch cover a launch at K (layout_mu held)
bool side_ready(const Plan::SpmmSide& S, u32 K) {
    return S.built && (S.partials == 0 || S.scratchK >= K);
}

// build (or rebuild for another chunk) one side's lists and size its scratch for K; layout_mu
// held. Synchronous on the plan's stream.
int build_side(const Plan& p, int side, u32 K, u32 chunk) {
    Plan::SpmmSide& S = p.spmm[side - 1];
    const hipStream_t s = p.stream;
    if (!S.built || (chunk != 0 && chunk != S.chunk)) {
        std::vector<u32> hrp, hci, hrows;
        BSMR_CHECK(p.rowptr.download(hrp, s));
        BSMR_CHECK(p.colidx.download(hci, s));
        SpmmIn in;
        in.M = p.M;
        in.N = p.N;
        in.nnz = p.nnz;
        in.rowptr = hrp.data();
        in.colidx = hci.data();
        in.side = side;
        in.chunk = chunk ? chunk : SPMM_CHUNK_DEFAULT;
        if (side == 1) {
            // rows in the plan's reordered order: a workgroup's waves share a panel's columns
            BSMR_CHECK(p.rows.download(hrows, s));
            hrows.resize(std::min<size_t>(hrows.size(), p.R));
            in.order = hrows.data();
            in.norder = static_cast<u32>(hrows.size());
        }
        SpmmLists L;
        std::string err;
        if (spmm_lists(in, L, err)) {
            set_error(std::string("bsmr_plan_prepare_spmm: ") + err);
            return BSMR_ERR_INVALID;
        }
        if (L.nSegs > (1ull << 31)) {
            set_error("bsmr_plan_prepare_spmm: more than 2^31 segments");
            return BSMR_ERR_UNSUPPORTED;
        }
        S.built = false;
        BSMR_CHECK(S.segs.upload(L.segs.data(), L.segs.size(), s));
        BSMR_CHECK(S.src.upload(L.src.data(), L.src.size(), s));
        BSMR_CHECK(S.vpos.upload(L.vpos.data(), L.vpos.size(), s));
        BSMR_CHECK(S.reds.upload(L.reds.data(), L.reds.size(), s));
        BSMR_HIP(hipStreamSynchronize(s));
        S.nSegs = static_cast<u32>(L.nSegs);
        S.nReds = static_cast<u32>(L.reds.size());
        S.splitDsts = L.splitDsts;
        S.partials = L.partials;
        S.maxList = L.maxList;
        S.chunk = L.chunk;
        S.scratch.release();
        S.scratchK = 0;
        S.built = true;
    }
    if (S.partials != 0 && S.scratchK < K) {
        S.scratchK = 0;
        BSMR_CHECK(S.scratch.alloc(static_cast<size_t>(S.partials) * K));
        S.scratchK = K;
    }
    return BSMR_OK;
}

int launch_side(const bsmr_plan* plan, int side, const float* dV, const void* dX, u32 K, int dtype,
                float* dY, void* stream) {
    const char* who = side_call(side);
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dV || !dX || !dY) {
        set_error(std::string(who) + ": null device pointer");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(report(validate_kd(who, K, dtype)));
    const Plan& p = plan->p;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Plan::SpmmSide& S = p.spmm[side - 1];
    SpmmArgs a{};
    const SpmmRed* reds = nullptr;
    u32 nReds = 0;
    {
        std::lock_guard<std::mutex> g(p.layout_mu);
        if (!side_ready(S, K)) {
            const LaunchSite at{s, who, "bsmr_plan_prepare_spmm", K, dtype};
            BSMR_CHECK(lazy_build_guard(at));
            BSMR_CHECK(build_side(p, side, K, 0));
        }
        a.segs = S.segs.data();
        a.src = S.src.data();
        a.vpos = S.vpos.data();
        a.partial = S.scratch.data();
        a.nSegs = S.nSegs;
        reds = S.reds.data();
        nReds = S.nReds;
    }
    a.V = dV;
    a.X = static_cast<const char*>(dX);
    a.Y = dY;
    a.K = K;
    a.rowBytes = K * (dtype == BSMR_F32 ? 4u : 2u);
    const u32 chunks = a.rowBytes / 16u;
    a.lanes = 1;
    while (a.lanes < chunks && a.lanes < 64u) a.lanes <<= 1;
    const SpmmFn fn = dtype == BSMR_F32   ? pick_spmm<BSMR_F32>(a.rowBytes)
                      : dtype == BSMR_F16 ? pick_spmm<BSMR_F16>(a.rowBytes)
                                          : pick_spmm<BSMR_BF16>(a.rowBytes);
    if (a.nSegs) {
        const u32 grid = (a.nSegs + SPMM_WAVES - 1) / SPMM_WAVES;
        hipLaunchKernelGGL(fn, dim3(grid), dim3(SPMM_WAVES * 64), 0, s, a);
        BSMR_HIP(hipGetLastError());
    }
    if (nReds) {
        const size_t threads = static_cast<size_t>(nReds) * (K / 4u);
        hipLaunchKernelGGL(k_spmm_reduce, dim3(static_cast<u32>((threads + 255) / 256)), dim3(256), 0, s, reds,
                           nReds, a.partial, dY, K);
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

}  // namespace
}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_spmm(const bsmr_plan* plan, const float* dV, const void* dB, uint32_t K, int dtype,
                         float* dY, void* stream) {
    return launch_side(plan, 1, dV, dB, K, dtype, dY, stream);
}

extern "C" int bsmr_spmm_t(const bsmr_plan* plan, const float* dV, const void* dA, uint32_t K, int dtype,
                           float* dY, void* stream) {
    return launch_side(plan, 2, dV, dA, K, dtype, dY, stream);
}

static int spmm_prepare_args(const char* who, const bsmr_plan* plan, uint32_t K, int sides) {
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    if (sides < 1 || sides > 3) {
        set_error(std::string(who) + ": sides must be 1 (rows), 2 (columns) or 3 (both)");
        return BSMR_ERR_INVALID;
    }
    return report(validate_kd(who, K, BSMR_F32));
}

extern "C" int bsmr_plan_prepare_spmm(const bsmr_plan* plan, uint32_t K, int sides, uint32_t chunk) {
    BSMR_CHECK(spmm_prepare_args("bsmr_plan_prepare_spmm", plan, K, sides));
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    for (int side = 1; side <= 2; ++side)
        if (sides & side) BSMR_CHECK(build_side(p, side, K, chunk));
    return BSMR_OK;
}

extern "C" int bsmr_plan_spmm_prepared(const bsmr_plan* plan, uint32_t K, int sides) {
    if (spmm_prepare_args("bsmr_plan_spmm_prepared", plan, K, sides) != BSMR_OK) return 0;
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    for (int side = 1; side <= 2; ++side)
        if ((sides & side) && !side_ready(p.spmm[side - 1], K)) return 0;
    return 1;
}

extern "C" int bsmr_plan_spmm_stats(const bsmr_plan* plan, int side, bsmr_spmm_stats* out) {
    if (!plan || !out || (side != 1 && side != 2)) {
        set_error("bsmr_plan_spmm_stats: null argument or side not 1 (rows) / 2 (columns)");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    const Plan::SpmmSide& S = p.spmm[side - 1];
    *out = bsmr_spmm_stats{};
    if (S.built) {
        out->segments = S.nSegs;
        out->split_dsts = S.splitDsts;
        out->partials = S.partials;
        out->max_list = S.maxList;
        out->chunk = S.chunk;
    }
    return BSMR_OK;
}
