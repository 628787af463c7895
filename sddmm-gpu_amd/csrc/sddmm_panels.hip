// sddmm_panels.hip — SDDMM over the plan's pattern for gfx950 on matrix instructions, per 16-row
// panel (bsmr_sddmm_mfma: P[e] = dot(A[row(e)], B[col(e)]) for fp16 / bf16 A and B, fp32 P at CSR
// positions). It is the first product of attention_panels.hip, S^T = B_tile
// A_panel^T under the step's mask, stored instead of fed to a softmax.
//
// Lists. Nothing of its own: the items and steps of panel_rows (attention_panels.hpp) and the rows
// side's base / pos of the panel SpMM (spmm_panels.hpp), which give the CSR position behind every
// mask bit. Each is built through its owner's builder when no earlier call built it.
//
// Work split. One launch. A workgroup of PANEL_WAVES waves takes one item; wave w takes the item's
// steps w, w + 4, ... (at most PANEL_ITEM_STEPS / PANEL_WAVES = 4 of them). SDDMM entries are
// independent, so a step is a complete piece of work whoever runs it: no partials, no reduce, and
// a split panel is nothing special. An item of 0 steps exits at once; a wave without a step helps
// to stage the panel's rows and exits behind the barrier. Nothing is written but the stored
// entries.
//
// The panel's rows. The 16 x K block of A is fetched once per workgroup: chunk x = 256 u + thread
// is 16 bytes of row x / (K / 8), so every row is read once, by 16-byte loads, and stored to LDS
// rows AROW = 2 K + 16 bytes apart behind one workgroup barrier (32.25 KiB at K = 1024). Rows past
// the end of a short last panel are zeros. Lane (r, g) then reads its B operand of k-step s, the
// 16 bytes of elements [32 s + 8 g, +8) of row r, at 32-bit word r (K / 2 + 4) + 16 s + 4 g. A
// 16-byte LDS read is served a quarter wave at a time (16 lanes of one g, 4 words each, on 64
// banks): within it the first words are r (K / 2 + 4) + const = 4 r (K / 8 + 1) + const, and K / 8
// is even for every K of the list, so 4 (K / 8 + 1) r runs over the 16 multiples of 4 (mod 64)
// as r runs over 0 .. 15: the 64 words of a quarter fall on 64 different banks. (Without the 16
// bytes of padding every row would start on bank 0 for K >= 128.) The padding also keeps the rows
// 16-byte aligned for the 16-byte stores. For K <= 256 a wave reads its K / 32 operands once
// (K / 8 registers) and keeps them for all its steps; for K = 512 and 1024 it walks K in chunks
// of 256 inside a step and reads the chunk's eight operands from LDS again per chunk.
//
// A step. The MFMA's A operand is the B row of tile column i: lane (i, g) loads the 16 bytes of
// elements [32 s + 8 g, +8) of rows cols[i] (tile 0) and cols[16 + i] (tile 1), one load per tile
// and k-step, from L2; every B row of a step is read once per step (four lanes, 64 contiguous
// bytes per k-step). The two accumulators of a step (f32x4 each) are carried through the chunks,
// so there is no grid dimension over K and the step record is read once. A unit is one chunk of
// one step; a wave's units run in order, and the 16 loads of unit u + 1 (the next chunk, or the
// next step's first) are issued before the MFMAs of unit u: two register sets of 64 at K >= 256.
// The wave's column indices, masks and bases (four steps at most) and then the loads of its first
// unit are issued ahead of the staging, so the B rows travel while the A rows are staged. The
// eight positions of a lane's set bits, pos[base[16 s + r] + popcount(mask_r below the slot)],
// are requested with the loads of the step's first chunk, one unit ahead of its MFMAs: they are
// needed only for the store (two sets of eight, by step parity). Lane (r, g) ends a step with the scores of panel row r at step slots
// panel_slot(g, j) (panel_mfma.hpp) and issues one 4-byte store per set mask bit; a clear bit
// (padding slots, rows past the panel's end) issues neither the position load nor the store.
//
// Summation order: k-steps of 32 ascending into one accumulator chain per tile, chunks ascending,
// inside a k-step the order of v_mfma_f32_16x16x32. It is fixed by (K, dtype) alone: the pattern,
// the item and the wave that runs a step do not enter it. P is the fp32 accumulator as it is.
//
// NaN / inf. Containment is exact: C[i][n] reads only B row cols[i] and A row n, so a non-finite
// value in a B row reaches exactly the entries that store that column and one in an A row exactly
// that row's entries. A padding slot repeats a column of its own step and is never stored.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "attention_common.hpp"
#include "attention_panels.hpp"
#include "launch_select.hpp"
#include "panel_host.hpp"
#include "panel_mfma.hpp"
#include "plan.hpp"

namespace bsmr {
namespace {

constexpr u32 SDDMM_MFMA_CHUNK = 256;                               // elements of K per unit
constexpr int SDDMM_MFMA_STEPS = PANEL_ITEM_STEPS / PANEL_WAVES;    // steps of an item per wave, at most

struct SddmmMfmaArgs {
    const PanelItem* items;
    const PanelStep* steps;
    const u32* rows;  // the launch order of the panel rows; null: the identity
    const u32* base;  // 16 per step
    const u32* pos;   // one per stored entry
    const char* A;    // M x K of the operand type
    const char* B;    // N x K
    float* P;         // nnz, CSR positions
    u32 M;
};

template <int DT, int K>
__global__ __launch_bounds__(PANEL_WAVES * 64) void k_sddmm_mfma(const SddmmMfmaArgs a) {
    constexpr int KC = K < static_cast<int>(SDDMM_MFMA_CHUNK) ? K : static_cast<int>(SDDMM_MFMA_CHUNK);
    constexpr int NCH = K / KC;             // chunks (units) per step
    constexpr int KS = KC / 32;             // k-steps per chunk
    constexpr int NU = SDDMM_MFMA_STEPS * NCH;
    constexpr u32 AROW = 2u * K + 16u;      // bytes between the staged A rows
    constexpr u32 CPR = K / 8;              // 16-byte chunks per row
    constexpr u32 ACHUNKS = PANEL_ROWS * CPR;
    constexpr u32 NT = PANEL_WAVES * 64;
    __shared__ __attribute__((aligned(16))) char astage[PANEL_ROWS * AROW];

    const PanelItem it = a.items[blockIdx.x];
    if (it.nsteps == 0) return;  // (the whole workgroup)
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 r = lane & 15u, g = lane >> 4;
    // steps wave, wave + 4, ... of the item
    const int mine = it.nsteps > wave ? static_cast<int>((it.nsteps - wave + PANEL_WAVES - 1) / PANEL_WAVES) : 0;

    // the wave's step records: tile columns of lane (i = r), the row's mask and base
    u32 c0[SDDMM_MFMA_STEPS], c1[SDDMM_MFMA_STEPS], mk[SDDMM_MFMA_STEPS], bs[SDDMM_MFMA_STEPS];
#pragma unroll
    for (int t = 0; t < SDDMM_MFMA_STEPS; ++t) {
        c0[t] = c1[t] = mk[t] = bs[t] = 0;
        if (t < mine) {
            const size_t s = static_cast<size_t>(it.step0) + wave + PANEL_WAVES * t;
            c0[t] = a.steps[s].cols[r];
            c1[t] = a.steps[s].cols[16u + r];
            mk[t] = a.steps[s].masks[r];
            bs[t] = a.base[s * PANEL_ROWS + r];
        }
    }

    const size_t brow = 2u * static_cast<size_t>(K);
    // unit u = chunk u % NCH of the wave's step u / NCH: its 2 KS operand loads and, with a step's
    // first chunk, the positions of the lane's set bits (needed only at the step's store)
    u32 pn[2][8];
    auto load_unit = [&](int u, uint4 (&b)[2 * KS]) {
        const int t = u / NCH, ch = u % NCH;
        const char* p0 = a.B + static_cast<size_t>(c0[t]) * brow + (static_cast<u32>(ch) * KC + 8u * g) * 2u;
        const char* p1 = a.B + static_cast<size_t>(c1[t]) * brow + (static_cast<u32>(ch) * KC + 8u * g) * 2u;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            b[2 * s] = load16(p0 + 64u * s);
            b[2 * s + 1] = load16(p1 + 64u * s);
        }
        if (ch == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const u32 c = panel_slot(g, j);
                pn[t & 1][j] = 0;
                if ((mk[t] >> c) & 1u)
                    pn[t & 1][j] = a.pos[static_cast<size_t>(bs[t]) + __builtin_popcount(mk[t] & ((1u << c) - 1u))];
            }
        }
    };
    uint4 bx[2 * KS], by[2 * KS];
    if (mine) load_unit(0, bx);  // in flight under the staging

    // the panel's A rows into LDS, once per workgroup
#pragma unroll
    for (u32 x0 = 0; x0 < ACHUNKS; x0 += NT) {
        const u32 x = x0 + threadIdx.x;
        if (ACHUNKS % NT == 0 || x < ACHUNKS) {
            const u32 pr = x / CPR, ch = x % CPR;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (it.row0 + pr < a.M) {
                const u32 row = a.rows ? a.rows[it.row0 + pr] : it.row0 + pr;
                v = load16(a.A + static_cast<size_t>(row) * (2u * K) + ch * 16u);
            }
            *reinterpret_cast<uint4*>(astage + pr * AROW + ch * 16u) = v;
        }
    }
    __syncthreads();
    if (mine == 0) return;

    const char* arow = astage + r * AROW + g * 16u;  // the lane's operand of k-step s: + 64 s
    uint4 q[KS];
    if constexpr (NCH == 1) {
#pragma unroll
        for (int s = 0; s < KS; ++s) q[s] = *reinterpret_cast<const uint4*>(arow + 64u * s);
    }

    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    auto run_unit = [&](int u, const uint4 (&b)[2 * KS]) {
        const int t = u / NCH, ch = u % NCH;
        if (ch == 0) acc0 = acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (NCH > 1) {
#pragma unroll
            for (int s = 0; s < KS; ++s) q[s] = *reinterpret_cast<const uint4*>(arow + 2u * KC * ch + 64u * s);
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            acc0 = mfma32<DT>(b[2 * s], q[s], acc0);
            acc1 = mfma32<DT>(b[2 * s + 1], q[s], acc1);
        }
        if (ch == NCH - 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((mk[t] >> panel_slot(g, j)) & 1u) a.P[static_cast<size_t>(pn[t & 1][j])] = j < 4 ? acc0[j] : acc1[j - 4];
        }
    };

    // the wave's units in order, the loads of the next one ahead of this one's MFMAs; unrolled, so
    // that the record arrays and the two register sets are indexed statically. (The positions of
    // step t wait in set t & 1: step t + 2 requests its own after step t's store.)
    const int units = mine * NCH;
#pragma unroll
    for (int u = 0; u < NU; u += 2) {
        if (u >= units) break;
        if (u + 1 < units) load_unit(u + 1, by);
        run_unit(u, bx);
        if (u + 1 >= units) break;
        if (u + 2 < NU && u + 2 < units) load_unit(u + 2, bx);
        run_unit(u + 1, by);
    }
}

using SddmmMfmaFn = void (*)(const SddmmMfmaArgs);

template <int DT>
SddmmMfmaFn pick_k(u32 K) {
    switch (K) {
        case 32: return k_sddmm_mfma<DT, 32>;
        case 64: return k_sddmm_mfma<DT, 64>;
        case 128: return k_sddmm_mfma<DT, 128>;
        case 256: return k_sddmm_mfma<DT, 256>;
        case 512: return k_sddmm_mfma<DT, 512>;
        default: return k_sddmm_mfma<DT, 1024>;
    }
}

constexpr const char* PREP = "bsmr_plan_prepare_sddmm_mfma";

// the row lists and the rows side's positions are built (layout_mu held)
bool lists_ready(const Plan& p) { return p.panel_rows.built && p.spmm_panels[0].built; }

int prepare_args(const char* who, const bsmr_plan* plan, u32 K) {
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    return report(validate_sddmm_mfma(who, K, BSMR_F16));  // (the prepare calls carry no dtype)
}

}  // namespace
}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_sddmm_mfma(const bsmr_plan* plan, const void* dA, const void* dB, uint32_t K, int dtype, float* dP,
                               void* stream) {
    const char* who = "bsmr_sddmm_mfma";
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dA || !dB || !dP) {
        set_error(std::string(who) + ": null device pointer");
        return BSMR_ERR_INVALID;
    }
    if (!attn_aligned16(dA) || !attn_aligned16(dB) || (reinterpret_cast<uintptr_t>(dP) & 3u)) {
        set_error(std::string(who) + ": dA and dB must be 16-byte aligned and dP 4-byte aligned");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(report(validate_sddmm_mfma(who, K, dtype)));
    const Plan& p = plan->p;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    SddmmMfmaArgs a{};
    u32 nItems = 0;
    {
        std::lock_guard<std::mutex> g(p.layout_mu);
        BSMR_CHECK(panel_build_missing(
            LaunchSite{s, who, PREP, K, dtype}, [&] { return lists_ready(p); },
            [&] { return std::string("the panel lists and the entry positions"); },
            [&] { return spmm_panels_build_positions(p, 1, PREP); }));
        a.items = p.panel_rows.items.data();
        a.steps = p.panel_rows.steps.data();
        a.rows = p.panel_rows.rows.data();
        a.base = p.spmm_panels[0].base.data();
        a.pos = p.spmm_panels[0].pos.data();
        nItems = p.panel_rows.nItems;
    }
    a.A = static_cast<const char*>(dA);
    a.B = static_cast<const char*>(dB);
    a.P = dP;
    a.M = p.M;
    if (nItems > 0x1FFFFFFFu) {
        set_error(std::string(who) + ": more than 2^29 items");
        return BSMR_ERR_UNSUPPORTED;
    }
    // one workgroup of PANEL_WAVES waves per item: panel_launch's count is in waves, and there is
    // no second launch
    void (*const none)(const SddmmMfmaArgs, const PanelRed*, u32) = nullptr;
    return panel_launch(s, dtype == BSMR_F16 ? pick_k<BSMR_F16>(K) : pick_k<BSMR_BF16>(K), a, nItems * PANEL_WAVES, dim3(1), none,
                        static_cast<const PanelRed*>(nullptr), 0u, 0u, dim3(1));
}

extern "C" int bsmr_plan_prepare_sddmm_mfma(const bsmr_plan* plan, uint32_t K) {
    BSMR_CHECK(prepare_args(PREP, plan, K));
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    return spmm_panels_build_positions(p, 1, PREP);
}

extern "C" int bsmr_plan_sddmm_mfma_prepared(const bsmr_plan* plan, uint32_t K) {
    if (prepare_args("bsmr_plan_sddmm_mfma_prepared", plan, K) != BSMR_OK) return 0;
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    return lists_ready(p) ? 1 : 0;
}

extern "C" int bsmr_plan_sddmm_mfma_stats(const bsmr_plan* plan, bsmr_sddmm_mfma_stats* out) {
    if (!plan || !out) {
        set_error("bsmr_plan_sddmm_mfma_stats: null argument");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    *out = bsmr_sddmm_mfma_stats{};
    if (lists_ready(p)) {
        const Plan::PanelListState& L = p.panel_rows;
        out->panels = L.panels;
        out->items = L.nItems;
        out->steps = L.nSteps;
        out->waves = p.spmm_panels[0].stepWaves;
        out->fill_permille = panel_fill_permille(p.nnz, L.nSteps);
    }
    return BSMR_OK;
}
