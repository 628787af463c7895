// spmm_panels.hip — SpMM over the plan's pattern for gfx950 on matrix instructions, per 16-destination
// panel (bsmr_spmm_panels: Y = S(V) B, rows of S; bsmr_spmm_t_panels: Y = S(V)^T A, columns of S;
// fp16 / bf16 dense operands, fp32 V and Y): the gradients dA / dB of bsmr_sddmm when V = dP.
//
// The gather kernel (spmm.hip) loads one dense row per stored entry and does one FMA per element.
// Here a wave takes an item of the panel lists (attention_panels.hpp; the rows side runs over the
// attention forward's lists, the columns side over the panel backward's): up to PANEL_ITEM_STEPS
// steps of 32 sources of one panel's union, every dense row of the union loaded once for the
// panel's 16 destinations. It is the second product of attention_panels.hip with its lane mapping
// (r = l & 15, g = l >> 4; panel_mfma.hpp), Y^T += X^T W^T per 16 columns of K:
//   weights  lane (r, g) owns destination r's eight weights of a step, step slots panel_slot(g, j)
//            (the k-slot order): the entry of slot c is V[pos[base[r] + popcount(mask_r below c)]]
//            (spmm_panels.hpp); a lane whose mask bit is clear issues no load and holds 0. Positions
//            and values of step s + 1 are requested before the MFMAs of step s;
//   pieces   an fp32 weight does not fit a 16-bit operand, and rounding it would lose a gradient of
//            1e-8 (0 in fp16) or 1e5 (inf), so it enters as several operands whose sum is the value:
//            fp16  per destination a running exponent m, the largest biased exponent of |V| seen so
//                  far (in-lane maximum and xor steps 16 and 32 over the row's four lanes); when m
//                  grows, acc is multiplied by 2^(m_old - m_new), exactly (ldexp); t = V 2^(127 - m)
//                  (exact, |t| < 2) is hi = fp16(t), lo = fp16(t - hi): two MFMAs per tile into one
//                  accumulator; the store multiplies by 2^(m - 127). m starts at 0, which is a scale
//                  like any other: a row of zeros keeps acc = 0 and stores 0, and no NaN appears;
//            bf16  has fp32's exponents and needs no scale: hi = bf16(V), mid = bf16(V - hi),
//                  lo = bf16(V - hi - mid) carry 8 + 8 + 8 significand bits, V = hi + mid + lo
//                  exactly: three MFMAs per tile;
//   X        the step's 32 dense rows (this slice's 2 KS bytes of each) are staged in LDS by 16-byte
//            loads, rows staged_row_bytes(KS) apart, and read through staged_pair: lane (r, g) ends
//            with Y[r][32 n + 8 g, +8).
// K <= 256 is one slice; 512 and 1024 run as slices of 256 columns in the grid's second dimension,
// each of which reads the step records and the values again and its own 512 bytes of every row.
// An item that is its panel's only one stores Y; an item of a split panel stores (m, acc) per row
// to plan-owned scratch and k_spmm_panels_reduce takes the largest m, scales every partial by an
// exact power of two and adds in item order. No atomics: the order is a function of the panel's
// union alone.
//
// Conventions: bsmr_spmm's, but a non-finite V[e] makes its whole destination row non-finite (hi or
// lo is inf or NaN for every column) and no other row, and a NaN or inf in a dense row reaches every
// destination of the panels whose union holds that row (0 x NaN inside the MFMA is NaN) and no
// destination of another panel.
//
// Resources: four waves per workgroup, one item each, 32 staged_row_bytes(KS) bytes of LDS per wave
// (66 KiB per workgroup at KS = 256: two workgroups per CU, amdgpu_waves_per_eu(2)).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "attention_common.hpp"
#include "attention_panels.hpp"
#include "panel_host.hpp"
#include "panel_mfma.hpp"
#include "plan.hpp"
#include "spmm_panels.hpp"

namespace bsmr {
namespace {

constexpr u32 SPMM_PANEL_SLICE = 256;  // columns of K per wave: 16 x 256 fp32 accumulators are 64 registers

struct SpmmPanelArgs {
    const PanelItem* items;
    const PanelStep* steps;
    const u32* rows;  // the launch order of the destinations; null: the identity (columns side)
    const u32* base;  // 16 per step
    const u32* pos;   // one per stored entry
    const float* V;
    const char* X;    // sources x K of the operand type
    float* Y;         // destinations x K
    float* pacc;      // partials x 16 x K
    int* pm;          // behind them: partials x 16 running exponents (fp16)
    u32 nItems, D, K;
};

template <int DT, int KS>
__global__ __launch_bounds__(PANEL_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2)))
void k_spmm_panels(const SpmmPanelArgs a) {
    constexpr int NP = KS / 32;                 // pairs of output tiles
    constexpr u32 XROW = staged_row_bytes(KS);  // bytes between staged rows
    constexpr u32 CPR = KS / 8;                 // 16-byte chunks per staged row
    constexpr int XLOADS = KS / 16;             // chunks per lane and step (32 rows)
    constexpr int XBATCH = XLOADS < 8 ? XLOADS : 8;
    __shared__ __attribute__((aligned(16))) char xstage[PANEL_WAVES][PANEL_STEP_COLS * XROW];

    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 itemId = blockIdx.x * PANEL_WAVES + wave;
    if (itemId >= a.nItems) return;
    const PanelItem it = a.items[itemId];
    const u32 k0 = blockIdx.y * KS;  // this slice's first column
    const size_t xrow = static_cast<size_t>(a.K) * 2u;
    const char* Xs = a.X + static_cast<size_t>(k0) * 2u;
    char* xl = xstage[wave];

    const u32 r = lane & 15u, g = lane >> 4;
    const bool live = it.row0 + r < a.D;  // (a row of a short last panel has no mask bit and is not stored)
    const u32 row = !live ? 0u : a.rows ? a.rows[it.row0 + r] : it.row0 + r;

    int m = 0;  // fp16: the running biased exponent of the row
    f32x4 acc[2 * NP];
#pragma unroll
    for (int n = 0; n < 2 * NP; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const PanelStep* st = a.steps + it.step0;
    const u32* bs = a.base + static_cast<size_t>(it.step0) * PANEL_ROWS;
    // a step's weights in two dependent rounds of loads, each predicated on the lane's mask bits
    auto load_pos = [&](const PanelStep* sp, const u32* bp, u32* p) {
        const u32 mask = sp->masks[r], b = bp[r];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const u32 c = panel_slot(g, j);
            p[j] = 0xFFFFFFFFu;
            if ((mask >> c) & 1u) p[j] = a.pos[b + __builtin_popcount(mask & ((1u << c) - 1u))];
        }
    };
    auto load_val = [&](const u32* p, float* w) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            w[j] = 0.f;
            if (p[j] != 0xFFFFFFFFu) w[j] = a.V[p[j]];
        }
    };
    u32 pn[8];
    float w[8], wn[8];
    if (it.nsteps) {
        load_pos(st, bs, pn);
        load_val(pn, w);
    }
    for (u32 step = 0; step < it.nsteps; ++step, ++st, bs += PANEL_ROWS) {
        const u32 colv = st->cols[lane & 31u];  // lane x holds step source x & 31
        const bool more = step + 1 < it.nsteps;
        if (more) load_pos(st + 1, bs + PANEL_ROWS, pn);

        // the step's dense rows into LDS: chunk x = 64 u + lane is 16 bytes of row x / CPR. The reads
        // of the step before are done first
        wave_lds_sync();
#pragma unroll
        for (int u0 = 0; u0 < XLOADS; u0 += XBATCH) {
            uint4 v[XBATCH];
#pragma unroll
            for (int u = 0; u < XBATCH; ++u) {
                const u32 x = 64u * (u0 + u) + lane;
                const u32 col = __shfl(colv, static_cast<int>(x / CPR));
                v[u] = load16(Xs + static_cast<size_t>(col) * xrow + (x % CPR) * 16u);
            }
#pragma unroll
            for (int u = 0; u < XBATCH; ++u) {
                const u32 x = 64u * (u0 + u) + lane;
                *reinterpret_cast<uint4*>(xl + (x / CPR) * XROW + (x % CPR) * 16u) = v[u];
            }
        }
        if (more) load_val(pn, wn);  // (the positions arrived under the row loads)

        // the weights as operands whose sum is the weight
        constexpr int PIECES = DT == BSMR_F16 ? 2 : 3;
        uint4 pb[PIECES];
        if constexpr (DT == BSMR_F16) {
            u32 amax = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = max(amax, __float_as_uint(w[j]) & 0x7FFFFFFFu);
            amax = max(amax, static_cast<u32>(__shfl_xor(static_cast<int>(amax), 16)));
            amax = max(amax, static_cast<u32>(__shfl_xor(static_cast<int>(amax), 32)));
            const int mn = max(m, static_cast<int>(amax >> 23));
            if (__builtin_amdgcn_ballot_w64(mn != m)) {  // wave-uniform: some row's scale grows
                const int d = m - mn;
#pragma unroll
                for (int n = 0; n < 2 * NP; ++n)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[n][e] = __builtin_ldexpf(acc[n][e], d);
            }
            m = mn;
            float hi[8], lo[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float t = __builtin_ldexpf(w[j], 127 - m);
                hi[j] = static_cast<float>(static_cast<_Float16>(t));
                lo[j] = t - hi[j];
            }
            pb[0] = pack8<DT>(hi);
            pb[1] = pack8<DT>(lo);
        } else {
            float hi[8], mid[8], lo[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                hi[j] = static_cast<float>(static_cast<__bf16>(w[j]));
                const float r1 = w[j] - hi[j];
                mid[j] = static_cast<float>(static_cast<__bf16>(r1));
                lo[j] = r1 - mid[j];
            }
            pb[0] = pack8<DT>(hi);
            pb[1] = pack8<DT>(mid);
            pb[2] = pack8<DT>(lo);
        }

        wave_lds_sync();
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            uint4 even, odd;
            staged_pair<XROW>(xl, n, r, g, even, odd);
#pragma unroll
            for (int q = 0; q < PIECES; ++q) {
                acc[2 * n] = mfma32<DT>(even, pb[q], acc[2 * n]);
                acc[2 * n + 1] = mfma32<DT>(odd, pb[q], acc[2 * n + 1]);
            }
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = wn[j];
        }
    }

    if (!live) return;
    // acc[2 n][j] and acc[2 n + 1][j] are columns 32 n + 8 g + 2 j and + 2 j + 1 of the row
    const bool direct = it.part == PANEL_DIRECT;
    const int back = DT == BSMR_F16 && direct ? m - 127 : 0;  // (ldexp by 0 changes nothing)
    float* o = direct ? a.Y + static_cast<size_t>(row) * a.K
                      : a.pacc + (static_cast<size_t>(it.part) * PANEL_ROWS + r) * a.K;
    o += k0 + 8u * g;
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        const f32x4 e = acc[2 * n], d = acc[2 * n + 1];
        *reinterpret_cast<float4*>(o + 32 * n) = make_float4(__builtin_ldexpf(e[0], back), __builtin_ldexpf(d[0], back),
                                                             __builtin_ldexpf(e[1], back), __builtin_ldexpf(d[1], back));
        *reinterpret_cast<float4*>(o + 32 * n + 4) = make_float4(__builtin_ldexpf(e[2], back), __builtin_ldexpf(d[2], back),
                                                                 __builtin_ldexpf(e[3], back), __builtin_ldexpf(d[3], back));
    }
    // (every slice finds the same m: the first one records it)
    if (DT == BSMR_F16 && !direct && g == 0 && blockIdx.y == 0) a.pm[static_cast<size_t>(it.part) * PANEL_ROWS + r] = m;
}

// a split panel's rows: fp16 (SCALED) takes the largest exponent of the items, scales every partial
// by 2^(m_i - m), exactly, and multiplies the sum by 2^(m - 127); both add in item order. One thread
// per row and four columns
template <bool SCALED>
__global__ __launch_bounds__(256) void k_spmm_panels_reduce(const SpmmPanelArgs a, const PanelRed* reds, u32 nReds) {
    const u32 q4 = a.K / 4u;
    const size_t t = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= static_cast<size_t>(nReds) * PANEL_ROWS * q4) return;
    const PanelRed rd = reds[t / (PANEL_ROWS * q4)];
    const u32 r = static_cast<u32>(t / q4) % PANEL_ROWS, q = static_cast<u32>(t % q4);
    if (rd.row0 + r >= a.D) return;
    const u32 row = a.rows ? a.rows[rd.row0 + r] : rd.row0 + r;
    const size_t slot0 = static_cast<size_t>(rd.part0) * PANEL_ROWS + r;  // partials are 16 slots apart
    const float4* p = reinterpret_cast<const float4*>(a.pacc + slot0 * a.K) + q;
    int m = 127;
    if (SCALED) {
        m = a.pm[slot0];
        for (u32 i = 1; i < rd.nparts; ++i) m = max(m, a.pm[slot0 + static_cast<size_t>(i) * PANEL_ROWS]);
    }
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (u32 i = 0; i < rd.nparts; ++i) {
        const int d = SCALED ? a.pm[slot0 + static_cast<size_t>(i) * PANEL_ROWS] - m : 0;
        const float4 x = p[static_cast<size_t>(i) * PANEL_ROWS * q4];
        const float fx = __builtin_ldexpf(x.x, d), fy = __builtin_ldexpf(x.y, d), fz = __builtin_ldexpf(x.z, d),
                    fw = __builtin_ldexpf(x.w, d);
        s.x = i ? s.x + fx : fx;
        s.y = i ? s.y + fy : fy;
        s.z = i ? s.z + fz : fz;
        s.w = i ? s.w + fw : fw;
    }
    const int back = m - 127;
    reinterpret_cast<float4*>(a.Y + static_cast<size_t>(row) * a.K)[q] =
        make_float4(__builtin_ldexpf(s.x, back), __builtin_ldexpf(s.y, back), __builtin_ldexpf(s.z, back), __builtin_ldexpf(s.w, back));
}

using SpmmPanelFn = void (*)(const SpmmPanelArgs);

template <int DT>
SpmmPanelFn pick_slice(u32 K) {
    switch (K) {
        case 32: return k_spmm_panels<DT, 32>;
        case 64: return k_spmm_panels<DT, 64>;
        case 128: return k_spmm_panels<DT, 128>;
        default: return k_spmm_panels<DT, 256>;  // 256, and 512 / 1024 in slices
    }
}

const char* side_call(int side) { return side == 1 ? "bsmr_spmm_panels" : "bsmr_spmm_t_panels"; }

// fp16 / bf16 and the row sizes the engine names; else BSMR_ERR_UNSUPPORTED with the message set
int spmm_panels_validate(const char* who, u32 K, int dtype) {
    const bool k = K == 32 || K == 64 || K == 128 || K == 256 || K == 512 || K == 1024;
    if ((dtype != BSMR_F16 && dtype != BSMR_BF16) || !k) {
        set_error(std::string(who) + ": dtype must be BSMR_F16 or BSMR_BF16 and K one of 32, 64, 128, 256, 512, 1024");
        return BSMR_ERR_UNSUPPORTED;
    }
    return BSMR_OK;
}

// a side's lists, positions and scratch cover a launch at K (layout_mu held)
bool side_ready(const Plan& p, int side, u32 K) {
    const Plan::SpmmPanelsSide& S = p.spmm_panels[side - 1];
    const Plan::PanelListState& L = p.panel_lists(side);
    return S.built && L.built && (L.partials == 0 || S.scratchK >= K);
}

// the side's lists and positions (panel_host.hpp) and its scratch for K: it grows and never shrinks;
// layout_mu held. Synchronous on the plan's stream.
int build_side(const Plan& p, int side, u32 K, const char* who) {
    BSMR_CHECK(spmm_panels_build_positions(p, side, who));
    Plan::SpmmPanelsSide& S = p.spmm_panels[side - 1];
    const Plan::PanelListState& L = p.panel_lists(side);
    if (L.partials != 0 && S.scratchK < K) {
        BSMR_CHECK(S.scratch.grow(attn_sat_mul(attn_sat_mul(L.partials, PANEL_ROWS), static_cast<size_t>(K) + 1u)));
        S.scratchK = K;
    }
    return BSMR_OK;
}

int launch_side(const bsmr_plan* plan, int side, const float* dV, const void* dX, u32 K, int dtype, float* dY, void* stream) {
    const char* who = side_call(side);
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dV || !dX || !dY) {
        set_error(std::string(who) + ": null device pointer");
        return BSMR_ERR_INVALID;
    }
    if (!attn_aligned16(dX) || !attn_aligned16(dY) || (reinterpret_cast<uintptr_t>(dV) & 3u)) {
        set_error(std::string(who) + ": the dense operand and dY must be 16-byte aligned");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(spmm_panels_validate(who, K, dtype));
    const Plan& p = plan->p;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    SpmmPanelArgs a{};
    const PanelRed* reds = nullptr;
    u32 nReds = 0;
    {
        std::lock_guard<std::mutex> g(p.layout_mu);
        const char* prep = "bsmr_plan_prepare_spmm_panels";
        BSMR_CHECK(panel_build_missing(
            LaunchSite{s, who, prep, K, dtype}, [&] { return side_ready(p, side, K); },
            [&] { return "the panel lists, the entry positions (or the scratch for K = " + std::to_string(K) + ")"; },
            [&] { return build_side(p, side, K, prep); }));
        const Plan::SpmmPanelsSide& S = p.spmm_panels[side - 1];
        const Plan::PanelListState& L = p.panel_lists(side);
        a.items = L.items.data();
        a.steps = L.steps.data();
        a.rows = L.rows.data();
        a.nItems = L.nItems;
        a.base = S.base.data();
        a.pos = S.pos.data();
        a.pacc = S.scratch.data();
        a.pm = a.pacc ? reinterpret_cast<int*>(a.pacc + static_cast<size_t>(L.partials) * PANEL_ROWS * K) : nullptr;
        reds = L.reds.data();
        nReds = L.nReds;
    }
    a.V = dV;
    a.X = static_cast<const char*>(dX);
    a.Y = dY;
    a.D = side == 1 ? p.M : p.N;
    a.K = K;
    const u32 slices = K > SPMM_PANEL_SLICE ? K / SPMM_PANEL_SLICE : 1u;
    const bool f16 = dtype == BSMR_F16;
    return panel_launch(s, f16 ? pick_slice<BSMR_F16>(K) : pick_slice<BSMR_BF16>(K), a, a.nItems, dim3(1, slices),
                        f16 ? k_spmm_panels_reduce<true> : k_spmm_panels_reduce<false>, reds, nReds, K / 4u, dim3(1));
}

int prepare_args(const char* who, const bsmr_plan* plan, u32 K, int sides) {
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    if (sides < 1 || sides > 3) {
        set_error(std::string(who) + ": sides must be 1 (rows), 2 (columns) or 3 (both)");
        return BSMR_ERR_INVALID;
    }
    return spmm_panels_validate(who, K, BSMR_F16);  // (the prepare calls carry no dtype)
}

}  // namespace

// panel_host.hpp: the side's lists (through their owner's builder) and its positions (once)
int spmm_panels_build_positions(const Plan& p, int side, const char* who) {
    Plan::SpmmPanelsSide& S = p.spmm_panels[side - 1];
    const hipStream_t s = p.stream;
    BSMR_CHECK(side == 1 ? attn_panels_build_lists(p, who) : attn_bwd_panels_build_col_lists(p, who));
    const Plan::PanelListState& L = p.panel_lists(side);
    if (S.built) return BSMR_OK;
    // the lists as the device holds them: what the kernel walks is what the positions follow
    std::vector<u32> hrp, hci, hrows, trp, tci, tpos, base, pos;
    std::vector<PanelStep> steps;
    std::vector<PanelItem> items;
    BSMR_CHECK(p.rowptr.download(hrp, s));
    BSMR_CHECK(p.colidx.download(hci, s));
    BSMR_CHECK(L.steps.download(steps, s));
    BSMR_CHECK(L.items.download(items, s));
    std::string err;
    int st;
    if (side == 1) {
        BSMR_CHECK(L.rows.download(hrows, s));
        st = spmm_panel_positions(p.M, p.N, hrp.data(), hci.data(), nullptr, hrows.data(), steps.data(), steps.size(),
                                  items.data(), items.size(), base, pos, err);
    } else {
        st = spmm_pattern_transpose_pos(p.M, p.N, hrp.data(), hci.data(), trp, tci, tpos, err);
        hrows.resize(p.N);
        for (u32 j = 0; j < p.N; ++j) hrows[j] = j;
        if (!st)
            st = spmm_panel_positions(p.N, p.M, trp.data(), tci.data(), tpos.data(), hrows.data(), steps.data(), steps.size(),
                                      items.data(), items.size(), base, pos, err);
    }
    if (st) {
        set_error(std::string(who) + ": " + err);
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(S.base.upload(base.data(), base.size(), s));
    BSMR_CHECK(S.pos.upload(pos.data(), pos.size(), s));
    BSMR_HIP(hipStreamSynchronize(s));
    u64 waves = 0;
    for (const PanelItem& it : items) waves += std::min(it.nsteps, PANEL_WAVES);
    S.stepWaves = static_cast<u32>(std::min<u64>(waves, 0xFFFFFFFFu));
    S.built = true;
    return BSMR_OK;
}

}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_spmm_panels(const bsmr_plan* plan, const float* dV, const void* dB, uint32_t K, int dtype, float* dY,
                                void* stream) {
    return launch_side(plan, 1, dV, dB, K, dtype, dY, stream);
}

extern "C" int bsmr_spmm_t_panels(const bsmr_plan* plan, const float* dV, const void* dA, uint32_t K, int dtype, float* dY,
                                  void* stream) {
    return launch_side(plan, 2, dV, dA, K, dtype, dY, stream);
}

extern "C" int bsmr_plan_prepare_spmm_panels(const bsmr_plan* plan, uint32_t K, int sides) {
    const char* who = "bsmr_plan_prepare_spmm_panels";
    BSMR_CHECK(prepare_args(who, plan, K, sides));
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    for (int side = 1; side <= 2; ++side)
        if (sides & side) BSMR_CHECK(build_side(p, side, K, who));
    return BSMR_OK;
}

extern "C" int bsmr_plan_spmm_panels_prepared(const bsmr_plan* plan, uint32_t K, int sides) {
    if (prepare_args("bsmr_plan_spmm_panels_prepared", plan, K, sides) != BSMR_OK) return 0;
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    for (int side = 1; side <= 2; ++side)
        if ((sides & side) && !side_ready(p, side, K)) return 0;
    return 1;
}

extern "C" int bsmr_plan_spmm_panels_stats(const bsmr_plan* plan, int side, bsmr_spmm_panels_stats* out) {
    if (!plan || !out || (side != 1 && side != 2)) {
        set_error("bsmr_plan_spmm_panels_stats: null argument or side not 1 (rows) / 2 (columns)");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    *out = bsmr_spmm_panels_stats{};
    const Plan::PanelListState& L = p.panel_lists(side);
    if (p.spmm_panels[side - 1].built && L.built)
        panel_list_stats(L, p.nnz, out->panels, out->items, out->steps, out->split_panels, out->partials, out->fill_permille);
    return BSMR_OK;
}
